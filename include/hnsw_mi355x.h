/*
 * hnsw_mi355x.h -- C ABI of libhnsw_mi355x.so: an MI355X-native (gfx950 / CDNA4) HNSW engine that
 * drops in behind the public API of the Rust `hnsw` crate of Gumo-A/hnsw_rs.
 *
 * The reference has no FFI seam of its own: callers link the `hnsw` crate and use
 * hnsw::template::HNSW directly.  The seam preserved here is that public Rust API; a same-named
 * Rust shim (shim-rust/, source only) binds these entry points -- see INTEGRATION.md.
 * Every entry point cites the reference item it replaces (paths relative to the reference
 * repository root).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every in/out buffer, nothing is retained
 *     after return; an opaque handle owns the host index and its HBM-resident snapshot.
 *   - every fallible call returns an int status (0 = HNSW_OK, < 0 = error); the text of the
 *     last error on the calling thread is available from hnsw_last_error().  Nothing unwinds or
 *     aborts across the ABI; where the reference panics (dim mismatch, NaN distance) the shim
 *     maps the status back to a panic, where it returns Err(String) to Err(String).
 *   - vectors are row-major float32; ids are the reference's NodeID = u32 (graph/src/lib.rs:1),
 *     dense 0..N-1 in insertion order (points/src/points.rs:64-73); UINT32_MAX pads id outputs.
 *   - search runs ONLY on the GPU (hand-written HIP, gfx950).  There is no CPU fallback: without
 *     a usable device the search entry points fail with HNSW_ERR_NO_DEVICE / HNSW_ERR_HIP.
 *   - concurrent searches on one handle are safe (the reference's ann_by_vector takes &self);
 *     insert_* must not run concurrently with anything else on the same handle.
 */
#ifndef HNSW_MI355X_H
#define HNSW_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define HNSW_OK 0
#define HNSW_ERR_BAD_DIM (-1)           /* template.rs:253-262 panics */
#define HNSW_ERR_NAN_INPUT (-2)         /* graph/src/dist.rs:32, vectors/src/quant.rs:44,48 panic */
#define HNSW_ERR_NODE_NOT_IN_GRAPH (-3) /* searcher.rs:45-50 Err(String) */
#define HNSW_ERR_IO (-4)                /* template.rs:75-93 Err(String) / save panics */
#define HNSW_ERR_HIP (-5)
#define HNSW_ERR_RCCL (-6)
#define HNSW_ERR_OOM (-7)
#define HNSW_ERR_ARG (-8)
#define HNSW_ERR_EMPTY (-9)             /* index has no points (template.rs:318 unwrap panics) */
#define HNSW_ERR_NO_DEVICE (-10)
#define HNSW_ERR_OVERFLOW (-11)         /* internal scratch exhausted even after the retry path */
#define HNSW_ERR_SELF_CONNECTION (-12)  /* graph/src/graph.rs:38-40 */

/* ---- vector kinds ------------------------------------------------------------------------- */
/* points/src/point.rs:4  `type VecType = QuantVec` is what the reference ships: 8-bit scalar
 * quantisation with on-the-fly dequantised f32 L2 (vectors/src/quant.rs).  HNSW_VEC_F32 is the
 * reference's alternate `VecType = FullVec` (vectors/src/full.rs). */
#define HNSW_VEC_QUANT8 0
#define HNSW_VEC_F32 1

typedef struct hnsw_index hnsw_index;

/* hnsw/src/params.rs:5-13 `pub struct Params` (a public field of HNSW, template.rs:37) */
typedef struct hnsw_params {
    uint32_t ep;
    uint32_t vec_kind;
    uint64_t m;
    uint64_t mmax;
    uint64_t mmax0;
    float ml;
    uint32_t _pad;
    uint64_t ef_cons;
    uint64_t dim;
} hnsw_params;

/* per-query traversal counters (the reference has none; they define the algorithmic bytes of
 * the roofline report): n_dist = distance evaluations (incl. the entry point), n_exp = expanded
 * candidates, sum_deg = sum of the degrees of the expanded adjacency rows. */
typedef struct hnsw_query_stats {
    uint32_t n_dist;
    uint32_t n_exp;
    uint32_t sum_deg;
    int32_t status; /* per-query status (HNSW_OK or an error code) */
} hnsw_query_stats;

const char *hnsw_last_error(void);
const char *hnsw_version(void);

/* ---- construction -------------------------------------------------------------------------- */
/* HNSW::new(m, ef_cons: Option<usize>, dim), template.rs:133-144; ef_cons == 0 means None
 * (defaults ef_cons = 2m, mmax = m, mmax0 = 2m, ml = 1/ln(m): params.rs:20-42). */
int hnsw_create(uint32_t m, uint32_t ef_cons, uint32_t dim, int vec_kind, hnsw_index **out);
void hnsw_free(hnsw_index *h);
/* #[derive(Clone)] on HNSW, template.rs:35 (benches clone the index, hnsw_benchmarks.rs:23).  The clone starts with
 * every option of hnsw_set_option as its parent holds it ("filter_exact_grouped" and "mask_set_cache_mb" included), on
 * the parent's device, with the parent's deleted ids and labels; its HBM snapshot and its counters are its own. */
int hnsw_clone(const hnsw_index *h, hnsw_index **out);

int hnsw_get_params(const hnsw_index *h, hnsw_params *out);
/* params.ep is a public field; the reference re-picks it in hash order at every store
 * (template.rs:283-290) -- here the default is the smallest id on the top layer. */
int hnsw_set_ep(hnsw_index *h, uint32_t ep);

/* ---- build --------------------------------------------------------------------------------- */
/* HNSW::insert_bulk(self, vectors: Vec<Vec<f32>>, nb_threads, verbose), template.rs:388-444.
 * rows is n x dim row-major (the shim flattens Vec<Vec<f32>> and checks every row length,
 * returning HNSW_ERR_BAD_DIM where template.rs:253-262 panics).  May be called repeatedly. */
int hnsw_insert_bulk(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads, int verbose);
/* same, with the level of every new point given explicitly (levels[n]; NULL = draw them).  The
 * reference draws levels from rand's StdRng re-seeded with 0 at every store
 * (points/src/points.rs:39-48,148-160); rand is not part of the reference tree, so
 * reproducible tests pass levels in. */
int hnsw_insert_bulk_levels(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads,
                            int verbose, const uint8_t *levels);
/* insert_bulk on the GPU (on-device build), batch-synchronous.  Per batch one
 * wave per point runs Inserter::build_insertion_results (inserter.rs:40-126: entry point, greedy
 * descent, search_layer(ef_cons) + select_heuristic per layer) against the graph in HBM and files one
 * reverse-edge request per selected neighbour; the requests are radix-sorted by target row and one
 * wave per row applies make_connections / prune_connections (template.rs:196-238: append, or keep
 * the cap's nearest), a third pass drops the reverse edges of what was pruned (graph.rs:72-94, a
 * node's last edge stays).  The host graph is read back once at the end.  Points of one batch do not
 * see each other (like the racing threads of the reference's multi-threaded insert_bulk), so the graph
 * is judged by recall and invariants, not by identity with the sequential build.  Needs m <= 128 and
 * ef_construction <= 512; nb_threads is used for the host-side parts (store, seed, read-back).
 * hnsw_set_option(h, "gpu_build", 2) routes hnsw_insert_bulk here; "gpu_build" = 1 selects the older
 * hybrid form (GPU searches, connect / prune on nb_threads host threads with the reference's locks). */
int hnsw_insert_bulk_device(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads,
                            int verbose, const uint8_t *levels);
/* The on-device build sharded over the GPUs of a node (BASELINE configs[4]): every rank calls this with
 * the SAME rows / levels on its own replica.  The insertion searches of each batch are split over the
 * ranks by position and what they produce travels as edge records through an all-gather; the connect / prune /
 * drop phases are split by row ownership (node id % world: a row's outcome depends on that row and its records
 * alone), the removals and the rows each owner changed travelling through further all-gathers of the size the
 * batch needs; the replicas are identical after every batch.  The collective is the caller's: d_send (one slot)
 * and d_recv (world slots) are device buffers of hnsw_sharded_slot_bytes() per slot, and
 * `allgather(ctx, bytes_per_rank)` (bytes_per_rank <= the slot size, a multiple of 64) must all-gather the FIRST
 * bytes_per_rank bytes of every rank's d_send into d_recv, rank r's at offset r * bytes_per_rank, and return 0
 * once d_recv is complete (RCCL through torch.distributed in hnsw_rs_amd/hnsw.py).  The library has synchronised
 * the device before it calls.  Every rank makes the same sequence of calls with the same sizes. */
typedef int (*hnsw_allgather_fn)(void *ctx, uint64_t bytes_per_rank);
uint64_t hnsw_sharded_slot_bytes(const hnsw_index *h, uint32_t world);
int hnsw_insert_bulk_sharded(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                             const uint8_t *levels, uint32_t rank, uint32_t world, void *d_send, void *d_recv,
                             uint64_t slot_bytes, hnsw_allgather_fn allgather, void *ctx);
/* HNSW::insert_vec(&mut self, &Vec<f32>) -> Result<NodeID, String>, template.rs:165-173.  The reference's callers
 * search right after it (eval_glove/src/main.rs:37-41): when the HBM snapshot is current it is PATCHED -- the new
 * vector row, its upper-layer base and the adjacency rows the insertion touched go to the device in one staging
 * copy and one kernel, the arrays growing by a device-to-device copy when they are full -- so an insertion costs
 * O(rows touched) and the next search finds the snapshot current (hnsw_get_stat "point_patches" / "uploads"). */
int hnsw_insert_vec(hnsw_index *h, const float *v, uint32_t *out_id);
int hnsw_insert_vec_level(hnsw_index *h, const float *v, int level /* < 0: draw */, uint32_t *out_id);

/* Adopt a prebuilt graph (e.g. one built by another implementation of the reference) instead of
 * building: points first, then layers 0,1,2,... as CSR over ascending node ids, then the ep.
 * hnsw_import_layer checks every row before it writes the first: a node or a neighbour that the levels do not
 * put on the layer is HNSW_ERR_NODE_NOT_IN_GRAPH, a row that holds its own node is HNSW_ERR_SELF_CONNECTION
 * (graph/src/graph.rs:38-40: no graph of the reference holds one; hnsw_last_error names the node), and a
 * refused call imports nothing. */
int hnsw_import_points(hnsw_index *h, const float *rows, uint64_t n, const uint8_t *levels);
int hnsw_import_layer(hnsw_index *h, uint32_t layer, uint64_t n_nodes, const uint32_t *node_ids,
                      const uint64_t *offsets, const uint32_t *nbrs);

/* ---- query (the hot path; HIP kernels) ------------------------------------------------------ */
/* HNSW::ann_by_vector(&self, &Vec<f32>, n, ef) -> Result<Vec<NodeID>, String>, template.rs:306-335.
 * ids[n]; *count = number of ids returned (< n when ef < n or the index is tiny).
 * No limit on ef, like the reference: up to 1024 the candidate list lives in one wave's registers; beyond that
 * list and visited set live in HBM scratch (hx_search_spill_kernel: the same results, one insertion at a time,
 * orders of magnitude slower -- meant for correctness at the reference's contract, not for throughput). */
/* Concurrent calls on one handle are COALESCED (the reference takes &self, so its callers are many threads each
 * blocked in its own call): the first caller to arrive leads a batch, callers arriving with the same (n, ef) before
 * it is launched park their query in the batch's pinned staging area and sleep; the leader launches one kernel for
 * all of them and wakes them with their ids.  Every query is still answered by its own wave, so a call returns
 * exactly what it would return alone.  A lone caller launches at once; a leader that has seen concurrency waits up
 * to "coalesce_us" (hnsw_set_option; default 30, 0 = never wait, < 0 = coalescing off) for the callers that were
 * woken together to come back; at most "coalesce_depth" (3) batches are on the GPU at a time and a batch holds at
 * most "coalesce_max" (1024) queries. */
int hnsw_search(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, uint32_t *ids,
                uint32_t *count);
/* Batched form (new; the reference answers one query per call): Q is nq x dim host memory,
 * ids nq x n (pad UINT32_MAX), dists nq x n or NULL (the distances the reference discards, pad
 * +inf), counts nq or NULL, stats nq or NULL.  Returns the first per-query error, if any. */
int hnsw_search_batch(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                      uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats);
/* Filtered k-NN (an extension: the reference has no filter): the n nearest among the ALLOWED ids.  Id i is allowed
 * iff i < min(allow_bits, hnsw_len) and bit (i & 63) of allow[i >> 6] is set; one mask serves every query of the call
 * (a mask made before later inserts leaves the new points out).  1 <= n <= 64 (n == 0: nothing is returned or
 * launched); ef' = max(ef, n, 1).  Outputs as hnsw_search_batch (ids pad UINT32_MAX, dists pad +inf); paths[nq] or
 * NULL receives how each query was answered:
 *   0  graph path: the upper layers as ann_by_vector (greedy, ef 1, unfiltered); layer 0 keeps a frontier of
 *      unexpanded keys and a result set of allowed keys, ef' each; a neighbour is admitted while the result set is
 *      not full or it is below the set's largest, and the walk stops when the frontier's head lies above a full
 *      result set's largest ("Filtered search").  Needs ef' <= 256, else HNSW_ERR_ARG.  With every id
 *      allowed and ef >= n it returns exactly hnsw_search_batch's ids, distances and counters.
 *   1  exact path: the top min(n, A) of the A allowed ids by (dist, id), in the index's own arithmetic (that of
 *      hnsw_brute_force); stats n_dist = A, n_exp = sum_deg = 0.  Taken by every query of a call when
 *      A <= "filter_exact_max" (hnsw_set_option).
 *   2  the exact path for a graph-path query whose visited set filled the largest table (32768 slots, 24576 ids,
 *      checked before each pass of up to 64 (f32) / 32 (8-bit) ids), instead of HNSW_ERR_OVERFLOW.
 * A == 0 gives count 0 for every query.  The cosine option applies to the queries first.  Per-query errors
 * (HNSW_ERR_NAN_INPUT) as hnsw_search_batch.  The handle's deleted ids (hnsw_mark_deleted) are never allowed: the
 * effective mask is allow AND NOT deleted, and the result equals the same call with that mask on a handle with
 * nothing deleted.  Masks resident in HBM across calls and a device-pointer form are hnsw_mask_set's, below; one-query
 * calls under a set's row and a label range that gather into one launch are hnsw_search_filtered's, further below (a
 * one-query call under a mask of its own, not in a set, does not gather).  Not
 * provided: filtered sharded search, the Rust shim's binding, and a label
 * range (hnsw_search_batch_filtered_range, below) combined with a per-call mask or a mask per query in one call (with a
 * row of a resident set it is hnsw_search_batch_filtered_set_range, below; a disjunction of label ranges is
 * hnsw_search_batch_filtered_ranges, below). */
int hnsw_search_batch_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                               const uint64_t *allow, uint64_t allow_bits, uint32_t *ids, float *dists,
                               uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths /* 0/1/2 or NULL */);
/* The same with an allow-list PER QUERY: a batch whose requests carry different filters in one call.  masks is
 * n_masks rows of W = ceil(allow_bits / 64) words, row-major and contiguous, each row a mask in the layout above (all
 * share allow_bits); mask_of[i] names query i's row, or is HNSW_MASK_NONE: no allow-list, every id < hnsw_len is
 * allowed (no all-ones mask is built for it).  n_masks == 0 with masks == NULL is legal when every query is
 * HNSW_MASK_NONE.  Query i's ids, distance bits, count, stats (status included) and path are exactly what
 * hnsw_search_batch_filtered returns for that query alone under mask mask_of[i] (HNSW_MASK_NONE: under an all-ones
 * mask over hnsw_len bits) on the same handle with the same options: n, ef', deleted ids, the cosine option and
 * per-query errors as there (the call returns the first per-query error, every other row is filled in).
 * The planner runs per mask: the host counts the admissible ids A_g of every mask some query names; the queries of a
 * mask with A_g <= "filter_exact_max" take the exact path (1), the others the graph path (0), and a graph-path query
 * that fills the largest visited table is answered by the exact path under its own mask (2).  ef' > 256 is
 * HNSW_ERR_ARG when at least one named mask takes the graph path.  Masks no query names are neither counted nor
 * compacted.  All graph-path queries of all masks share ONE kernel launch (one wave per query, each wave reads its own
 * mask); the exact path runs once per named exact-path mask over that mask's queries.
 * HNSW_ERR_ARG, decided before the device is touched: Q, ids or mask_of NULL; masks NULL while allow_bits > 0 and some
 * query names a mask; a mask_of[i] that is neither < n_masks nor HNSW_MASK_NONE; n > 64; nq > 2^31 - 1.  nq == 0 is
 * HNSW_OK; n == 0 zeroes counts and launches nothing.  hnsw_get_stat: the three "filtered_*" counters advance by the
 * queries answered on each path, "filtered_multi_calls" by one and "filtered_multi_masks" by the masks named
 * (HNSW_MASK_NONE counts as one). */
#define HNSW_MASK_NONE 0xFFFFFFFFu
int hnsw_search_batch_filtered_multi(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                     const uint64_t *masks, uint32_t n_masks, uint64_t allow_bits,
                                     const uint32_t *mask_of /* nq */, uint32_t *ids, float *dists, uint32_t *counts,
                                     hnsw_query_stats *stats, uint8_t *paths /* 0/1/2 or NULL */);

/* ---- resident mask sets ------------------------------------------------------------------------------------------
 * Allow-lists that live with the index: n_masks rows of W = ceil(allow_bits / 64) words in the layout above, created
 * once, updated in place, named by searches and read in HBM -- the filter-side counterpart of hnsw_mark_deleted's
 * resident deny mask.  allow_bits is fixed at creation and may exceed hnsw_len (room for the ids of later inserts); an
 * id is admissible iff it is below min(allow_bits, hnsw_len), its bit is set and it is not deleted.  Bits of a row's
 * last word beyond allow_bits are ignored on input and read back as 0.
 *   create   masks: n_masks x W words, or NULL: every row clear
 *   write    replaces a whole row by words[W]
 *   update   sets (allow != 0) or clears the bits of ids[k] in one row; idempotent; an id >= allow_bits or a row >=
 *            n_masks is HNSW_ERR_ARG and the set stays as it was
 *   read     the row's words[W];   count: its set bits (below allow_bits);   info: n_masks and allow_bits
 * None of these needs a GPU: they work on a host mirror and note the words they changed.  The next search that names
 * the set brings the HBM copy up to date on the snapshot's device, by the deleted set's mechanism: the changed words
 * travel as (index, value) pairs and are scattered by one small kernel, or the whole set is copied when there is no
 * HBM copy yet, the device changed or more than an eighth of its words changed ("mask_set_words_uploaded").
 * A set belongs to the handle that created it (any other handle passed with it: HNSW_ERR_ARG); hnsw_clone, hnsw_save
 * and snapshot replication do not carry it; it must not be used after hnsw_free and is freed by its creator.  A
 * device-only replica may create sets (its length is the header's).  Concurrent searches that name one set are safe;
 * write and update must not run concurrently with a search on that set.
 * The set also keeps, per row, what a filtered call otherwise works out every time, valid while the row, the
 * handle's deleted set and hnsw_len are unchanged: the row's admissible count and word offsets (counted on the host
 * when a search first names the row: "mask_set_recounts"), and, for a row planned on the exact path, its compacted
 * ascending id list in HBM -- while that is valid a call launches the scan and the merge for the row and NO
 * compaction ("mask_set_compactions" counts the compactions that do run).  The lists of a set are bounded by the
 * option "mask_set_cache_mb"; when that is used up further rows are compacted per call as without a set, and nothing
 * is evicted. */
typedef struct hnsw_mask_set hnsw_mask_set;
int hnsw_mask_set_create(hnsw_index *h, uint32_t n_masks, uint64_t allow_bits,
                         const uint64_t *masks /* n_masks x W, or NULL: all clear */, hnsw_mask_set **out);
void hnsw_mask_set_free(hnsw_mask_set *s);
int hnsw_mask_set_info(const hnsw_mask_set *s, uint32_t *n_masks, uint64_t *allow_bits);
int hnsw_mask_set_write(hnsw_mask_set *s, uint32_t row, const uint64_t *words /* W */);
int hnsw_mask_set_update(hnsw_mask_set *s, uint32_t row, const uint32_t *ids, uint64_t k, int allow);
int hnsw_mask_set_read(const hnsw_mask_set *s, uint32_t row, uint64_t *words /* W */);
int hnsw_mask_set_count(const hnsw_mask_set *s, uint32_t row, uint64_t *allowed /* set bits below allow_bits */);
/* hnsw_search_batch_filtered_multi with the masks taken from a set: query i's ids, distance bits, count, stats (status
 * included) and path are exactly what that call returns for the same Q, n, ef and mask_of on the same handle with the
 * same options, its masks being the set's current rows (as hnsw_mask_set_read gives them) and its allow_bits the
 * set's -- HNSW_MASK_NONE, the per-mask planner, "filter_exact_max", ef' > 256, deleted ids, the cosine option and
 * per-query errors included.  mask_of == NULL: every query under row 0.  No mask is uploaded and no row the set has
 * counted is counted again; an exact-path row with a valid list is not compacted.  Argument errors as there, decided
 * before the device is touched, and HNSW_ERR_ARG for a NULL set or a set of another handle.  The three "filtered_*"
 * path counters advance as there, and "filtered_set_calls" by one. */
int hnsw_search_batch_filtered_set(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                   hnsw_mask_set *set, const uint32_t *mask_of /* nq; NULL: every query row 0 */,
                                   uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                                   uint8_t *paths /* 0/1/2 or NULL */);
/* The same with every buffer in HBM on the handle's device (d_mask_of too; NULL: row 0).  The set is brought up to
 * date on a stream of the handle's own, so `stream` is not synchronised; then ONE launch of the filtered graph kernel
 * for all queries is enqueued on `stream` and the call returns.  Every query takes the graph path: n <= 64 and
 * ef' <= 256, else HNSW_ERR_ARG.  d_stats is required; d_dists / d_counts may be NULL.  The host never sees d_mask_of
 * before the launch, so the kernel checks it: a query whose entry is neither < n_masks nor HNSW_MASK_NONE gets status
 * HNSW_ERR_ARG, count 0 and padded outputs without a mask word being read; every other query is answered as usual.
 * _finish (same arguments, and paths: host, nq, or NULL) waits for `stream`, reads the statuses and d_mask_of back,
 * re-runs the queries whose visited table filled up with larger tables, answers those that fill the largest by the
 * exact path under their own rows (path 2, with the set's caches) and returns the first per-query error.  After it the
 * buffers hold what hnsw_search_batch_filtered_set returns with "filter_exact_max" = -1 (paths 0 or 2); the counters
 * advance at _finish. */
int hnsw_search_batch_filtered_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                      hnsw_mask_set *set, const uint32_t *d_mask_of /* device, nq; NULL: row 0 */,
                                      uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                      hnsw_query_stats *d_stats, void *stream);
int hnsw_search_batch_filtered_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                             hnsw_mask_set *set, const uint32_t *d_mask_of, uint32_t *d_ids,
                                             float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                             void *stream, uint8_t *paths /* host, nq, or NULL */);

/* ---- labels and label-range filtered search ----------------------------------------------------------------------
 * A resident LABEL COLUMN: one uint32 per id (a tenant, a category, a timestamp), kept with the handle on the host and
 * in HBM, and searches filtered by a closed range over it -- the form a filter usually arrives in, with no mask built,
 * uploaded or stored for it (4 bytes per id, whatever the number of distinct predicates).  An id
 * whose label was never set has label 0, ids added by later inserts included.  Setting labels touches the host
 * mirror only and needs no GPU; the next range search brings the HBM copy up to date by the deleted set's mechanism:
 * the changed 64-bit words (two labels each) scattered by one small kernel, or one whole copy when there is no copy
 * yet, the device changed or more than an eighth of the words changed ("label_words_uploaded").  hnsw_clone and
 * hnsw_set_device carry the column, hnsw_save writes it as the file `labels` (see hnsw_save); hnsw_snapshot_describe /
 * _adopt do not carry it, but a device-only replica may set labels of its own (its length is the header's).
 * hnsw_set_labels must not run concurrently with a range search on the handle.
 * A range combined with a row of a resident mask set in one call is hnsw_search_batch_filtered_set_range, below; a
 * disjunction of up to HNSW_RANGES_MAX ranges per query (an IN-list) is hnsw_search_batch_filtered_ranges, below.
 * Not provided: a range combined with a mask that is not in a set, several label columns or labels that are not
 * integers, a range list combined with a mask row, range lists over shards, the Rust shim's binding, filtered sharded
 * search. */
/* labels[k] for ids[k]; ids == NULL: ids 0..k-1.  An id >= hnsw_len is HNSW_ERR_ARG and nothing changes.  Needs no GPU. */
int hnsw_set_labels(hnsw_index *h, const uint32_t *ids, const uint32_t *labels, uint64_t k);
/* out[k]: the labels of ids[k] (NULL: of ids 0..k-1); an id >= hnsw_len is HNSW_ERR_ARG */
int hnsw_get_labels(const hnsw_index *h, const uint32_t *ids /* NULL: 0..k-1 */, uint64_t k, uint32_t *out);
/* k-NN among the ids whose label lies in the query's own closed range: query i's ids, distance bits, count, stats
 * (status included) and path are exactly what hnsw_search_batch_filtered returns for that query alone, on the same
 * handle with the same options, under the mask {id < hnsw_len : lo[i] <= label(id) <= hi[i]} -- n <= 64,
 * ef' = max(ef, n, 1), deleted ids, the cosine option, per-query errors, path 2 on a visited-table overflow and
 * A == 0 giving count 0 as there.  Equality is [x, x], no filter is [0, UINT32_MAX]; lo[i] > hi[i] is an empty range:
 * count 0, status HNSW_OK, not an error.
 * The planner runs per distinct (lo, hi) pair named in the call: the host determines the range's admissible count A
 * exactly (two binary searches in a sorted copy of the column, which is made again when a label, the deleted set or
 * hnsw_len changed); a range with A <= "filter_exact_max" takes the exact path (1) once, over its queries, the others
 * the graph path (0), so the paths are those of the equivalent hnsw_search_batch_filtered_multi call.  ef' > 256 is
 * HNSW_ERR_ARG when some range takes the graph path.  All graph-path queries of all ranges share ONE launch of the
 * filtered graph kernel, each wave testing labels against its own range.
 * HNSW_ERR_ARG, decided before the device is touched: Q, ids, lo or hi NULL; n > 64; nq > 2^31 - 1.  nq == 0 is
 * HNSW_OK; n == 0 zeroes counts and launches nothing.  hnsw_get_stat: the three "filtered_*" path counters advance as
 * for _multi, "filtered_range_calls" by one and "filtered_range_ranges" by the distinct ranges named. */
int hnsw_search_batch_filtered_range(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                     const uint32_t *lo /* nq */, const uint32_t *hi /* nq */,
                                     uint32_t *ids, float *dists, uint32_t *counts,
                                     hnsw_query_stats *stats, uint8_t *paths /* 0/1/2 or NULL */);
/* The same with every buffer in HBM on the handle's device, d_lo and d_hi too (both required), after
 * hnsw_search_batch_filtered_device: the column is brought up to date on a stream of the handle's own, then ONE launch
 * of the filtered graph kernel is enqueued on `stream` and the call returns without synchronising.  Every query takes
 * the graph path: n <= 64 and ef' <= 256, else HNSW_ERR_ARG.  d_stats is required; d_dists / d_counts may be NULL.
 * _finish (same arguments, and paths: host, nq, or NULL) waits for `stream`, reads the statuses and d_lo / d_hi back,
 * re-runs the queries whose visited table filled up with larger tables, answers those that fill the largest by the
 * exact path under their own range (path 2) and returns the first per-query error.  After it the buffers hold what
 * hnsw_search_batch_filtered_range returns with "filter_exact_max" = -1 (paths 0 or 2); the counters advance at
 * _finish. */
int hnsw_search_batch_filtered_range_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                            const uint32_t *d_lo, const uint32_t *d_hi, uint32_t *d_ids,
                                            float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                            void *stream);
int hnsw_search_batch_filtered_range_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                   uint32_t ef, const uint32_t *d_lo, const uint32_t *d_hi,
                                                   uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                                   hnsw_query_stats *d_stats, void *stream,
                                                   uint8_t *paths /* host, nq, or NULL */);

/* ---- a label range AND a row of a resident mask set ---------------------------------------------------------------
 * The conjunction a filter usually is ("tenant == t AND visible under ACL row r", "timestamp in the last hour AND not
 * in this user's seen list"), with both halves read where they already are, in HBM: no conjunction mask is built,
 * uploaded or counted word by word on the host.  Query i's ids, distance bits, count, stats
 * (status included) and path are exactly what hnsw_search_batch_filtered returns for that query alone, on the same
 * handle with the same options, under the mask
 *   { id < min(set.allow_bits, hnsw_len) : bit id of row mask_of[i] is set AND lo[i] <= label(id) <= hi[i] }
 * -- for mask_of[i] == HNSW_MASK_NONE the first condition is id < hnsw_len -- with the deleted ids taken out, and
 * everything else as in _set and _range: n <= 64, ef' = max(ef, n, 1), the cosine option, per-query errors, A == 0
 * giving count 0, lo[i] > hi[i] an empty range and no error, path 2 on an overflow of the largest visited table.
 * mask_of == NULL: every query under row 0.  With every range [0, UINT32_MAX] the call returns what
 * hnsw_search_batch_filtered_set returns for the same mask_of, with every mask_of[i] == HNSW_MASK_NONE what
 * hnsw_search_batch_filtered_range returns for the same ranges.
 * The planner runs per distinct (row, lo, hi) triple named in the call and decides exactly: a triple takes the exact
 * path (1) iff its admissible count A <= "filter_exact_max", so the paths are those of the equivalent
 * hnsw_search_batch_filtered_multi call.  A is counted on the host by walking the cheaper side -- the range's slice of
 * the column's sorted copy, testing the row's bits, or the row's set bits, testing labels -- and only until it exceeds
 * "filter_exact_max": a triple on the graph path is not counted further (when one of its queries reaches path 2 it is
 * counted then).  A triple whose range is [0, UINT32_MAX] is planned as the row alone, with the set's caches; a
 * HNSW_MASK_NONE triple as the range alone.  The set's per-row caches (count, offsets, compacted list) describe the
 * row alone: a triple with a proper range neither reads them as its own nor invalidates them, and is compacted in the
 * call's scratch.  ef' > 256 is HNSW_ERR_ARG when some triple takes the graph path.  All graph-path queries of all
 * triples share ONE launch of the filtered graph kernel, each wave testing labels against its own range and bits of
 * its own row; the exact path runs once per exact-path triple.
 * HNSW_ERR_ARG, decided before the device is touched: Q, ids, set, lo or hi NULL; a set of another handle; a
 * mask_of[i] that is neither < n_masks nor HNSW_MASK_NONE; n > 64; nq > 2^31 - 1.  nq == 0 is HNSW_OK; n == 0 zeroes
 * counts and launches nothing.  hnsw_get_stat: the three "filtered_*" path counters advance as for _multi,
 * "filtered_set_range_calls" by one and "filtered_set_range_groups" by the distinct (row, lo, hi) triples named. */
int hnsw_search_batch_filtered_set_range(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                         hnsw_mask_set *set, const uint32_t *mask_of /* nq; NULL: every query row 0 */,
                                         const uint32_t *lo /* nq */, const uint32_t *hi /* nq */, uint32_t *ids,
                                         float *dists, uint32_t *counts, hnsw_query_stats *stats,
                                         uint8_t *paths /* 0/1/2 or NULL */);
/* The same with every buffer in HBM on the handle's device, after hnsw_search_batch_filtered_device and
 * _filtered_range_device: d_lo and d_hi are required, d_mask_of may be NULL (row 0).  The set and the column are
 * brought up to date on a stream of the handle's own, then ONE launch of the filtered graph kernel is enqueued on
 * `stream` and the call returns without synchronising.  Every query takes the graph path: n <= 64 and ef' <= 256, else
 * HNSW_ERR_ARG.  d_stats is required; d_dists / d_counts may be NULL.  A query whose d_mask_of entry is neither
 * < n_masks nor HNSW_MASK_NONE gets status HNSW_ERR_ARG, count 0 and padded outputs, and no mask word or label is read
 * for it.  _finish (same arguments, and paths: host, nq, or NULL) waits for `stream`, reads the statuses and d_mask_of
 * / d_lo / d_hi back, re-runs the queries whose visited table filled up with larger tables, answers those that fill the
 * largest by the exact path under their own (row, range) (path 2) and returns the first per-query error.  After it
 * the buffers hold what hnsw_search_batch_filtered_set_range returns with "filter_exact_max" = -1 (paths 0 or 2); the
 * counters advance at _finish. */
int hnsw_search_batch_filtered_set_range_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                                hnsw_mask_set *set, const uint32_t *d_mask_of /* device, nq; NULL: row 0 */,
                                                const uint32_t *d_lo, const uint32_t *d_hi, uint32_t *d_ids,
                                                float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                                void *stream);
int hnsw_search_batch_filtered_set_range_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                       uint32_t ef, hnsw_mask_set *set, const uint32_t *d_mask_of,
                                                       const uint32_t *d_lo, const uint32_t *d_hi, uint32_t *d_ids,
                                                       float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                                       void *stream, uint8_t *paths /* host, nq, or NULL */);

/* ---- label-SET filtered search: several label ranges per query ---------------------------------------------------
 * The disjunction over the label column -- `category IN (3, 7, 12)`, `tenant IN {a, b}`, "the last hour OR pinned" --
 * without a union mask built on the host, uploaded or stored.  Every query has n_ranges = K
 * closed ranges, fixed stride and row-major: query i is under [lo[i K + j], hi[i K + j]], j < K, and an id is allowed
 * iff its label lies in AT LEAST ONE of them.  A member with lo > hi is empty and is the padding: a ragged batch pads
 * its short lists with (1, 0).  Members may overlap, repeat, touch and come in any order; all members empty gives count
 * 0 with status HNSW_OK.  Query i's ids, distance bits, count, stats (status included) and path are exactly what
 * hnsw_search_batch_filtered returns for that query alone, on the same handle with the same options, under the mask
 *   { id < hnsw_len : label(id) in the union of query i's ranges }
 * and everything else is as in hnsw_search_batch_filtered_range: n <= 64, ef' = max(ef, n, 1), deleted ids taken out,
 * the cosine option, per-query errors, path 2 on an overflow of the largest visited table, A == 0 giving count 0.  With
 * n_ranges == 1 the call returns what hnsw_search_batch_filtered_range returns for the same lo / hi, launch for launch.
 * The host brings every query's list into its canonical form -- empty members dropped, the others sorted, overlapping
 * and adjacent ones merged ([1, 2], [3, 4] is [1, 4]; nothing is adjacent above UINT32_MAX) -- and the planner runs per
 * distinct canonical list named in the call: two raw lists with one canonical form are one group, and a list equal to
 * [0, UINT32_MAX] is no filter.  A is exact, the sum over the list's disjoint members of their slices of the column's
 * sorted copy; a list takes the exact path (1) iff A <= "filter_exact_max", once, over its queries, so the paths are
 * those of the equivalent hnsw_search_batch_filtered_multi call.  ef' > 256 is HNSW_ERR_ARG when some list takes the
 * graph path.  All graph-path queries of all lists share ONE launch of the filtered graph kernel, each wave testing
 * labels against its own list (the members as the caller gave them: no offsets, nothing canonical travels).
 * HNSW_ERR_ARG, decided before the device is touched: Q, ids, lo or hi NULL; n_ranges 0 or > HNSW_RANGES_MAX; n > 64;
 * nq > 2^31 - 1.  nq == 0 is HNSW_OK; n == 0 zeroes counts and launches nothing.  hnsw_get_stat: the three "filtered_*"
 * path counters advance as for _multi, "filtered_ranges_calls" by one and "filtered_ranges_groups" by the distinct
 * canonical lists named.
 * Not provided: a range list combined with a mask row, range lists over shards, the Rust shim's binding. */
#define HNSW_RANGES_MAX 16
int hnsw_search_batch_filtered_ranges(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                      uint32_t n_ranges, const uint32_t *lo /* nq x n_ranges */,
                                      const uint32_t *hi /* nq x n_ranges */, uint32_t *ids, float *dists,
                                      uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths /* 0/1/2 or NULL */);
/* The same with every buffer in HBM on the handle's device, d_lo and d_hi too (nq x n_ranges each, both required), after
 * hnsw_search_batch_filtered_range_device: the column is brought up to date on a stream of the handle's own, then ONE
 * launch of the filtered graph kernel is enqueued on `stream` and the call returns without synchronising.  There are
 * no offsets, so the kernel has nothing to validate.  Every query takes the graph path: n <= 64 and ef' <= 256, else
 * HNSW_ERR_ARG.  d_stats is required; d_dists / d_counts may be NULL.  _finish (same arguments, and paths: host, nq, or
 * NULL) waits for `stream`, reads the statuses and d_lo / d_hi back, re-runs the queries whose visited table filled up
 * with larger tables, answers those that fill the largest by the exact path under their own list (path 2) and returns
 * the first per-query error.  After it the buffers hold what hnsw_search_batch_filtered_ranges returns with
 * "filter_exact_max" = -1 (paths 0 or 2); the counters advance at _finish. */
int hnsw_search_batch_filtered_ranges_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                             uint32_t n_ranges, const uint32_t *d_lo, const uint32_t *d_hi,
                                             uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                             hnsw_query_stats *d_stats, void *stream);
int hnsw_search_batch_filtered_ranges_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                    uint32_t ef, uint32_t n_ranges, const uint32_t *d_lo,
                                                    const uint32_t *d_hi, uint32_t *d_ids, float *d_dists,
                                                    uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream,
                                                    uint8_t *paths /* host, nq, or NULL */);
/* ONE query under a filter, from many threads: the filtered form of hnsw_search.  The query is answered among the
 * undeleted ids below hnsw_len whose label lies in [lo, hi] ([0, UINT32_MAX]: no label filter) and, with a set, whose bit
 * is set in row `row` of it (HNSW_MASK_NONE: no row; set == NULL needs row == HNSW_MASK_NONE).  The ids, the distance
 * bits, *count, *path and the return value are exactly those of the one-query batch call on the same handle with the same
 * options -- set == NULL: hnsw_search_batch_filtered_range(h, q, 1, n, ef, &lo, &hi, ...); else
 * hnsw_search_batch_filtered_set_range(h, q, 1, n, ef, set, &row, &lo, &hi, ...) -- whatever the call was gathered with:
 * deleted ids, the cosine option, "filter_exact_max", ef' = max(ef, n, 1) <= 256 on the graph path, path 2 and A == 0
 * as there.  Concurrent calls on a handle gather exactly as hnsw_search calls do ("coalesce_us", "coalesce_depth",
 * "coalesce_max"; with "coalesce_us" < 0 every call launches by itself), in batches of their own: calls with equal
 * (n, ef, set) share a batch whatever their rows and ranges, never with hnsw_search calls.  The leader answers its batch
 * by one filtered search: the graph-path queries share ONE launch, the exact-path queries of ALL their groups one
 * compaction, one scan and one merge (the grouped form of the exact path; the batch entry points
 * use it with the option "filter_exact_grouped"), path 2 one more such pass.  A per-query error (HNSW_ERR_NAN_INPUT)
 * reaches only its caller.  dists (n floats) and path may be NULL.
 * HNSW_ERR_ARG, decided before the device is touched: h, q, ids or count NULL; n > 64; set == NULL with a row; a set of
 * another handle; a row that is neither < n_masks nor HNSW_MASK_NONE.  n == 0 gives *count = 0 and launches nothing.
 * hnsw_get_stat: "filtered_one_calls" (calls answered), "filtered_one_batches" (their leaders' launches); the three
 * "filtered_*" path counters advance as for the batch forms, whose "*_calls" and "*_groups" keys do not.
 * Not provided: one-query calls under a mask that is not in a set or under a list of ranges, the Rust shim's binding,
 * filtered search over shards. */
int hnsw_search_filtered(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, hnsw_mask_set *set /* or NULL */,
                         uint32_t row /* HNSW_MASK_NONE: no row */, uint32_t lo, uint32_t hi, uint32_t *ids,
                         float *dists /* or NULL */, uint32_t *count, uint8_t *path /* or NULL */);
/* The planner's own count: the undeleted ids below hnsw_len whose label lies in the union of the k <= HNSW_RANGES_MAX
 * ranges [lo[j], hi[j]] (a member with lo > hi is empty; k == 0 or all members empty gives 0) -- the selectivity a
 * caller wants before choosing ef.  Needs no GPU: it reads the column's sorted copy.  HNSW_ERR_ARG: h or count NULL,
 * lo or hi NULL while k > 0, k > HNSW_RANGES_MAX. */
int hnsw_count_labels_in_ranges(const hnsw_index *h, const uint32_t *lo, const uint32_t *hi, uint32_t k,
                                uint64_t *count);

/* hnsw_search_batch with every buffer already resident in HBM on the handle's device; enqueues on `stream`
 * (a hipStream_t, NULL = default stream) and returns without synchronising.  d_stats is
 * required (its status field carries per-query errors); d_dists / d_counts may be NULL.
 * The call can be captured in a graph as ONE kernel launch -- it allocates nothing, copies nothing and synchronises
 * nothing -- while all of these hold: the HBM snapshot is current (a search or hnsw_upload ran on the handle since the
 * last insert or option change), no id is deleted, the cosine option is off, ef <= 256 (lists of at most four
 * registers: longer ones take a second visited level in stream-ordered scratch on some paths) and the visited table
 * the launch starts with is at most 32 KiB of LDS (ef * max(mmax0, 8) / 32 <= 320, which ef <= 256 implies up to
 * mmax0 = 40, the default mmax0 = 2m at m <= 20).  Outside them the call brings state up to date, goes through the
 * filtered kernel's path, opts into more LDS or takes stream-ordered scratch, and is not promised to be capturable.  A
 * captured call cannot be completed by _finish inside the graph: the replaying caller inspects d_stats[i].status
 * itself. */
int hnsw_search_batch_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                             hnsw_query_stats *d_stats, void *stream);

/* Completes a hnsw_search_batch_device call (same arguments): waits for `stream`, reads the per-query
 * statuses, re-runs the queries whose visited table filled up with a larger table (the results are those a
 * larger table would have given from the start) and returns the first remaining per-query error -- the
 * error behaviour of the reference's `Result` (template.rs:306, 323) for callers that keep everything in
 * HBM.  The device entry above never synchronises; a caller that skips this call must inspect
 * d_stats[i].status itself. */
int hnsw_search_batch_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                    uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                    hnsw_query_stats *d_stats, void *stream);

/* ---- partitioned search: one index cut into shards ------------------------------------------------------------------
 * An extension (the reference keeps one index in one process's RAM, template.rs:35-40): the points are split over S
 * shards, each an ordinary index with ids local to it; every shard answers every query and the S result lists of a
 * query are merged into its n best.  Global id = id_base[s] + id_stride[s] * local id (contiguous blocks: base = the
 * block's first id, stride 1; round robin: base = s, stride = S).  This serves an index larger than one GPU's HBM (one
 * shard per rank; the lists arrive by RCCL's gather / all-gather, which produce the layout below) and segments on one
 * GPU (new data in a new small index next to immutable old ones).
 * THE MERGE of one query: over the present entries of all shards collect the pairs (distance bits as uint32, global
 * id); drop duplicates of a pair (overlapping shards may hand in the same point twice: it appears once); sort ascending
 * by the pair; keep n; pad the rest (ids UINT32_MAX, dists +inf).  Distances are non-negative, so bit order is value
 * order.  n_dist, n_exp and sum_deg are the uint32 sums over the shards; status is that of the lowest-numbered shard
 * whose status is not HNSW_OK, else HNSW_OK; a query whose merged status is not HNSW_OK gets count 0 and padded rows.
 *
 * hnsw_merge_topk_device is that merge alone, handle-free, on the current HIP device: every d_* pointer is device
 * memory, id_base / id_stride are host arrays of n_shards entries (id_stride NULL: all 1) and travel by value in the
 * kernel's arguments.  Inputs are shard-major: d_ids_in[S][nq][n] (local ids, pad UINT32_MAX), d_dists_in[S][nq][n],
 * d_counts_in[S][nq] or NULL, d_stats_in[S][nq] or NULL.  Entry j of shard s's list is present iff j < min(count, n),
 * or, without counts, iff its id is not UINT32_MAX.  The call enqueues ONE launch (the exact path's merge kernel in
 * its shard-list form, one wave per query) on `stream` and returns: it allocates nothing, copies nothing and
 * synchronises nothing, so it can be captured in a graph.  Outputs must not overlap inputs.  d_counts may be NULL;
 * d_stats is required iff d_stats_in is given.  THE CALLER GUARANTEES id_base[s] + id_stride[s] * id < UINT32_MAX for
 * every id shard s can return (the sum is taken in 32 bits and all 32 are used: ids at or above 2^31 are fine).
 * HNSW_ERR_ARG, decided before the device is touched: n_shards 0 or > HNSW_MERGE_MAX_SHARDS; n 0 or > 64;
 * nq > 2^31 - 1; d_ids_in, d_dists_in, id_base, d_ids or d_dists NULL; exactly one of d_stats_in / d_stats given.
 * nq == 0 is HNSW_OK, whatever else is passed, and launches nothing.
 *
 * hnsw_search_batch_shards answers host-pointer queries from S handles of one dimension on one device as from one
 * index: Q goes up once; each shard runs hnsw_search_batch_device into its slice of one [S][nq][n] scratch and then its
 * _finish, so overflow re-runs and the cosine option are each shard's own, unchanged; one merge; one copy back.  A
 * shard with deleted ids is answered by its hnsw_search_batch instead, the planner's choice of path ("filter_exact_max")
 * included, and its lists go up into its slice: the device entry point always walks the graph under deletions, and
 * the call is defined by the host form.  Query i's result is, by definition, THE MERGE of what each shard's
 * hnsw_search_batch returns for it, on the same handles with the same options.  Returns
 * the first per-query error; every other row is filled in.  Outputs as hnsw_search_batch (dists, counts, stats may be
 * NULL).  HNSW_ERR_ARG, decided before the device is touched: shards or id_base NULL, n_shards 0 or > 64, a NULL
 * handle, handles of differing dimension, handles bound to different devices (a handle not bound yet goes where the
 * others are), n > 64, nq > 2^31 - 1, Q or ids NULL; an empty shard is HNSW_ERR_EMPTY.  nq == 0 is HNSW_OK; n == 0
 * zeroes counts and launches nothing.  hnsw_get_stat on shard 0's handle: "shard_calls", "shard_merges".
 * Not provided: shards of one process on several GPUs; a partitioned build (a caller builds S ordinary indexes);
 * the filtered entry points over shards; n > 64; rebalancing; the Rust shim's binding. */
#define HNSW_MERGE_MAX_SHARDS 64
int hnsw_merge_topk_device(uint32_t n_shards, uint64_t nq, uint32_t n,
                           const uint32_t *d_ids_in, const float *d_dists_in,
                           const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                           const uint32_t *id_base /* S */, const uint32_t *id_stride /* S, or NULL: all 1 */,
                           uint32_t *d_ids, float *d_dists, uint32_t *d_counts /* or NULL */,
                           hnsw_query_stats *d_stats /* required iff d_stats_in */, void *stream);
int hnsw_search_batch_shards(hnsw_index *const *shards, uint32_t n_shards,
                             const uint32_t *id_base, const uint32_t *id_stride /* or NULL */,
                             const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats);

/* ---- grouped search: the nearest groups by label, at most per_group hits per group --------------------------------
 * An extension (the reference has no labels).  When the vectors are chunks, frames or sentences and the label
 * (hnsw_set_labels) is the parent's id, the caller wants the n_groups nearest distinct labels with their per_group best
 * hits each, not the nearest chunks (Qdrant's search groups, Milvus's grouping search, Elasticsearch's collapse).
 * THE COLLAPSE of one query's candidate list of `pool` entries (id_j, dist_j), j < pool, in the order given (the search
 * calls hand them over ascending by (distance bits, id), but the collapse is defined by position and sorts nothing):
 *   - entry j is PRESENT iff j < min(count, pool), or, without counts, iff id_j != UINT32_MAX; absent entries take no
 *     part, wherever they are;
 *   - lab_j is the handle's label of id_j as of the call (an id at or beyond the column's length has label 0; a handle
 *     on which no label was ever set has every label 0: one group);
 *   - the RANK r_j is the number of present i < j with lab_i == lab_j; the FIRST MEMBER f_j the smallest present i with
 *     lab_i == lab_j; the GROUP INDEX g_j the number of present i < f_j with r_i == 0 -- groups are numbered in the
 *     order of their first, that is best, member;
 *   - entry j is KEPT iff r_j < per_group and g_j < n_groups, and is written to slot [g_j][r_j].
 * Per query: ids [n_groups][per_group] (pad UINT32_MAX), dists [n_groups][per_group] (the distance bits of the input,
 * pad +inf), group_labels [n_groups] (pad 0), group_sizes [n_groups] (min(per_group, entries of that label in the
 * pool), pad 0), counts = min(n_groups, distinct labels present).  A query's stats record passes through unchanged;
 * a query whose incoming status is not HNSW_OK gets count 0 and fully padded rows.
 * Limits: 1 <= pool <= HNSW_GROUP_POOL_MAX; 1 <= n_groups, per_group <= pool; n_groups * per_group <= 1024.
 *
 * hnsw_group_by_label_device is the collapse alone over lists in HBM: every d_* pointer is device memory, the inputs
 * d_ids_in / d_dists_in [nq][pool], d_counts_in [nq] or NULL, d_stats_in [nq] or NULL are what any *_device search of
 * the same handle leaves after its _finish (ids local to the handle; lists merged over shards carry global ids and are
 * out of scope).  The label column's HBM copy is brought up to date on a stream of the handle's own, exactly as the
 * _range_device entry points do it; then ONE launch (the exact path's merge kernel in its collapse form, one wave per
 * query) is enqueued on `stream` and the call returns without synchronising `stream`.  Outputs must not overlap
 * inputs.  d_counts may be NULL; d_stats is required iff d_stats_in is given.  HNSW_ERR_ARG, decided before the device
 * is touched: h NULL; the limits above violated; nq > 2^31 - 1; d_ids_in, d_dists_in, d_ids, d_dists, d_group_labels
 * or d_group_sizes NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK on any handle, whatever else is
 * passed, and launches nothing; an empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_grouped answers host-pointer queries by their nearest groups.  By definition the result is THE
 * COLLAPSE of the candidate lists that an existing call returns with n = pool, on the same handle with the same
 * options: hnsw_search_batch (set NULL, lo and hi NULL), hnsw_search_batch_filtered_range (lo and hi), _filtered_set
 * (set; mask_of NULL: row 0) or _filtered_set_range (both).  Everything of the candidate call is inherited: ef' =
 * max(ef, n, 1), deleted ids taken out, the cosine option, the planner and "filter_exact_max", path 2, its stats, its
 * per-query errors (the first is returned, every other row is filled in) and its limits -- pool <= 64 and, on the
 * graph path, ef' <= 256 whenever the candidate call is a filtered one or the handle has deleted ids.  Unfiltered with
 * nothing deleted the call runs on the device end to end: the queries go up once, hnsw_search_batch_device and its
 * _finish, the collapse, one copy of the grouped block back.  Under a filter or deletions the candidates come from
 * the candidate call's HOST form and their lists go up before the collapse: only the host form lets the planner choose
 * the exact path, and the call is defined by it.  dists, group_sizes, counts and stats may be NULL.  HNSW_ERR_ARG,
 * decided before the device is touched: the limits violated; mask_of without a set; exactly one of lo / hi; a set of
 * another handle; Q, ids or group_labels NULL; nq > 2^31 - 1.  nq == 0 is HNSW_OK.  hnsw_get_stat: "grouped_calls",
 * "grouped_launches".
 * Not provided: grouping over shards; a refill loop when fewer than n_groups groups are in the pool (the caller raises
 * pool); a group key other than the label column; a device-resident filtered path; one-query gathered calls; the Rust
 * shim's binding. */
#define HNSW_GROUP_POOL_MAX 256
int hnsw_group_by_label_device(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_groups, uint32_t per_group,
                               const uint32_t *d_ids_in /* nq x pool */, const float *d_dists_in,
                               const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                               uint32_t *d_ids, float *d_dists /* nq x n_groups x per_group */,
                               uint32_t *d_group_labels, uint32_t *d_group_sizes /* nq x n_groups */,
                               uint32_t *d_counts /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                               void *stream);
int hnsw_search_batch_grouped(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_groups, uint32_t per_group,
                              uint32_t pool, uint32_t ef, hnsw_mask_set *set /* or NULL */,
                              const uint32_t *mask_of /* nq, or NULL */,
                              const uint32_t *lo, const uint32_t *hi /* nq each, or both NULL: no range */,
                              uint32_t *ids, float *dists /* or NULL */, uint32_t *group_labels,
                              uint32_t *group_sizes /* or NULL */, uint32_t *counts /* or NULL */,
                              hnsw_query_stats *stats /* or NULL */);

/* ---- radius search: every neighbour within a distance, found by a doubling ladder ---------------------------------
 * An extension (the reference answers "the n nearest" only): near-duplicate detection, score-threshold retrieval
 * (Qdrant's score_threshold, FAISS's range_search), clustering.
 * THE CUT of one query's candidate list of n_in entries (id_j, dist_j), j < n_in, at its radius, in the order given (the
 * cut is defined by position and sorts nothing):
 *   - entry j is PRESENT iff j < min(count, n_in), or, without counts, iff id_j != UINT32_MAX; absent entries take no
 *     part, wherever they are;
 *   - a present entry is KEPT iff dist_j <= radius, an f32 compare: a NaN distance is never kept, a NaN radius keeps
 *     nothing;
 *   - the w kept entries go to ids [0, w) and dists [0, w) in their input order, with the input's distance bits; slots
 *     [w, n_out) are padded with UINT32_MAX and +inf; counts = w;
 *   - flags has HNSW_RADIUS_MORE set iff the status is HNSW_OK, the number of present entries equals n_in and every
 *     present entry was kept: the list was full and showed nothing outside the radius, so there may be more.
 * A query's stats record passes through unchanged; a query whose incoming status is not HNSW_OK gets count 0, a padded
 * row and flags 0.  Limits: 1 <= n_in <= n_out <= HNSW_RADIUS_MAX_N (beyond 1024 entries the candidate list of a search
 * leaves the wave's registers for the spill kernel, orders of magnitude slower).
 *
 * hnsw_radius_cut_device is THE CUT alone over lists in HBM: every d_* pointer is device memory on the current device
 * (the call needs no handle, as hnsw_merge_topk_device), the inputs d_ids_in / d_dists_in [nq][n_in], d_counts_in [nq]
 * or NULL, d_stats_in [nq] or NULL are what any *_device search leaves after its _finish, d_radius [nq] the radii.  With
 * d_sel, n_sel entries naming queries below nq, launch block b serves query d_sel[b] and the rows of every other query
 * are not touched (an entry at or beyond nq is not served; a query named twice is written twice with the same words);
 * without, all nq are served.  Every output word of a served query is written exactly once.  ONE launch (the exact
 * path's merge kernel in its cut form, one wave per served query) is enqueued on `stream`; nothing is allocated, copied
 * or synchronised.  Outputs must not overlap inputs.  d_counts and d_flags may be NULL; d_stats is required iff
 * d_stats_in is given.  HNSW_ERR_ARG, decided before the device is touched: the limits violated; nq > 2^31 - 1;
 * d_radius, d_ids_in, d_dists_in, d_ids or d_dists NULL; d_sel given together with n_sel > nq; exactly one of d_stats_in
 * / d_stats given.  nq == 0 is HNSW_OK and launches nothing; so is d_sel given with n_sel == 0.
 *
 * hnsw_search_batch_radius answers host-pointer queries by THE LADDER, defined by existing calls.  Rung k has n_k =
 * min(n_first << k, max_n) and ef_k = max(ef, n_k); L_k(q) is what hnsw_search_batch returns for the original query
 * with n = n_k and ef = ef_k on the same handle with the same options: its ids, distance bits, count and stats.  Query q
 * stops at the first rung k at which its status is not HNSW_OK, or THE CUT of L_k(q) does not set HNSW_RADIUS_MORE, or
 * n_k == max_n.  Its answer is THE CUT of that L_k(q) at stride max_n: ids and dists [nq][max_n], counts = w, stats that
 * rung's record, rungs = k + 1, and flags keeps HNSW_RADIUS_MORE only in the third case, where it means "truncated at
 * max_n".  The first per-query error is returned, every other row is filled in.  Everything of the candidate call is
 * inherited: the cosine option (the radius is in the unit of the returned distances), deletions, overflow re-runs.
 * While ids are deleted hnsw_search_batch is the filtered search: max_n <= 64 is required, and max(ef, n_k) <= 256
 * whenever the graph path is taken.  Unfiltered with nothing deleted the call stays on the device: the queries go up
 * once (their unit-length copy under the cosine option is made once), every rung is one search launch over the
 * unfinished queries, its overflow re-runs and one cut launch over the same queries into the final block, only the nq
 * flag words come back between rungs, and the final block comes back in one copy.  While ids are deleted each rung's
 * candidates come from the HOST form of hnsw_search_batch on the unfinished queries and their lists go up before the
 * same cut: only the host form lets the planner choose the exact path.  dists, counts, flags, rungs and stats may be
 * NULL.  HNSW_ERR_ARG, decided before the device is touched: 1 <= n_first <= max_n <= HNSW_RADIUS_MAX_N violated (a
 * call has at most 11 rungs); Q, radius or ids NULL; nq > 2^31 - 1; a radius that is negative or NaN (+inf is legal);
 * max_n > 64 while ids are deleted.  nq == 0 is HNSW_OK; an empty index is HNSW_ERR_EMPTY.  hnsw_get_stat:
 * "radius_calls", "radius_rungs", "radius_launches".
 * Not provided: a radius inside the walk (the walk is the candidate call's, unchanged); CSR output from C (the Python
 * package's to_csr makes it); filters other than deletions; radius search over shards; one-query gathered calls; the
 * Rust shim's binding. */
#define HNSW_RADIUS_MAX_N 1024
#define HNSW_RADIUS_MORE  1u
int hnsw_radius_cut_device(uint64_t nq, uint32_t n_in, uint32_t n_out,
                           const float *d_radius /* nq */, const uint32_t *d_sel /* or NULL */, uint64_t n_sel,
                           const uint32_t *d_ids_in, const float *d_dists_in /* nq x n_in */,
                           const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                           uint32_t *d_ids, float *d_dists /* nq x n_out */, uint32_t *d_counts /* or NULL */,
                           uint32_t *d_flags /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                           void *stream);
int hnsw_search_batch_radius(hnsw_index *h, const float *Q, uint64_t nq, const float *radius /* nq */,
                             uint32_t n_first, uint32_t max_n, uint32_t ef,
                             uint32_t *ids /* nq x max_n */, float *dists /* or NULL */, uint32_t *counts /* or NULL */,
                             uint32_t *flags /* or NULL */, uint32_t *rungs /* or NULL */,
                             hnsw_query_stats *stats /* or NULL */);

/* ---- diversified search: hits near the query and not near each other (maximal marginal relevance) -----------------
 * An extension (the reference answers "the n nearest" only): near-duplicate rows, re-posts and boilerplate chunks fill a
 * top n with one answer n times; a retrieval caller wants MMR (LangChain's max_marginal_relevance_search, Qdrant's and
 * OpenSearch's MMR re-rank).  Grouped search removes duplicates by label; this removes them by distance, and it is the
 * one post-processing form that reads stored rows.
 * THE SELECTION out of one query's candidate list of `pool` entries (id_j, dist_j), j < pool, in the order given (the
 * selection sorts nothing), with the call's lambda in [0, 1] (f32) and output length n_out:
 *   - entry j is PRESENT iff j < min(count, pool), or, without counts, iff id_j != UINT32_MAX; absent entries take no
 *     part, wherever they are;
 *   - a present id at or beyond the index length gives the query status HNSW_ERR_ARG, count 0 and padded rows, and no row
 *     of the index is read for it;
 *   - the PAIR DISTANCE D(s, j) is the index's own distance between the stored rows id_s and id_j, the selected row s as
 *     the first argument: the bits of hnsw_distance(h, id_s, id_j) (Point::dist2other; under the cosine option the
 *     stored rows are the unit rows).  The routine is bit-symmetric for both vector kinds, but
 *     the argument order is part of the contract either way;
 *   - r_t(j) is the running minimum of D(s, j) over the entries s selected before step t, folded in selection order as
 *     `r = D < r ? D : r` from +inf (a NaN pair distance leaves it as it is); m_0(j) = 0 and m_t(j) = r_t(j) for t >= 1;
 *   - score_t(j) = (lambda * dist_j) - ((1.0f - lambda) * m_t(j)): three separately rounded f32 operations, never
 *     contracted, so numpy float32 restates them;
 *   - step t = 0, 1, ... < n_out selects the present, not yet selected entry with the smallest score under f32 `<`;
 *     entries equal under `==` (-0 == +0) go to the lower position j.  An entry whose score is NaN is never selected;
 *     when nothing is selectable the selection ends.
 * So lambda = 1 returns the first n_out present entries by (dist, position), and lambda = 0 starts at the first present
 * position and then walks farthest-point-first.  Per query, in selection order: ids [n_out] (pad UINT32_MAX), dists
 * [n_out] (the distance bits of the input, pad +inf), gaps [n_out] (r_t of the entry at the step t it was selected:
 * its distance to the nearest hit returned before it; gaps[0] = +inf; pad +inf), counts = entries selected.  A query's
 * stats record passes through unchanged (but for the status above); a query whose incoming status is not HNSW_OK gets
 * count 0 and padded rows.  Limits: 1 <= n_out <= pool <= HNSW_DIVERSE_POOL_MAX.
 *
 * hnsw_diversify_device is THE SELECTION alone over lists in HBM: every d_* pointer is device memory, the inputs
 * d_ids_in / d_dists_in [nq][pool], d_counts_in [nq] or NULL, d_stats_in [nq] or NULL are what any *_device search of
 * the same handle leaves after its _finish (ids local to the handle, so a replica handle serves as well: the rows read
 * are the snapshot's).  ONE launch (the distance seam's kernel in its selection form, one wave per query) is enqueued on
 * `stream` and the call returns without synchronising it; nothing is allocated or copied on it.  The status of an
 * out-of-range id is written to d_stats only (the call cannot see it).  Outputs must not overlap inputs.  d_gaps and
 * d_counts may be NULL; d_stats is required iff d_stats_in is given.  HNSW_ERR_ARG, decided before the device is
 * touched: h NULL; the limits violated; lambda outside [0, 1] or NaN; nq > 2^31 - 1; d_ids_in, d_dists_in, d_ids or
 * d_dists NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK on any handle, whatever else is passed,
 * and launches nothing; an empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_diverse answers host-pointer queries by n diverse hits each.  By definition the result is THE
 * SELECTION, with n_out = n, of the candidate lists that an existing call returns with n = pool, on the same handle
 * with the same options: hnsw_search_batch (set NULL, lo and hi NULL), hnsw_search_batch_filtered_range (lo and hi),
 * _filtered_set (set; mask_of NULL: row 0) or _filtered_set_range (both) -- the table of hnsw_search_batch_grouped, and
 * everything of the candidate call is inherited in the same way: ef' = max(ef, pool, 1), deleted ids taken out, the
 * cosine option, the planner and "filter_exact_max", its stats, its per-query errors (the first is returned, every
 * other row is filled in) and its limits -- pool <= 64 and, on the graph path, ef' <= 256 whenever the candidate call is
 * a filtered one or the handle has deleted ids.  Unfiltered with nothing deleted the call stays on the device: the
 * queries go up once, hnsw_search_batch_device and its _finish, one selection launch, one copy of the result block
 * back.  Under a filter or deletions the candidates come from the candidate call's HOST form and their lists go up
 * before the selection: only the host form lets the planner choose the exact path, and the call is defined by it.
 * dists, gaps, counts and stats may be NULL.  HNSW_ERR_ARG, decided before the device is touched: the limits violated;
 * lambda outside [0, 1] or NaN; mask_of without a set; exactly one of lo / hi; a set of another handle; Q or ids NULL;
 * nq > 2^31 - 1.  nq == 0 is HNSW_OK.  hnsw_get_stat: "diverse_calls" (hnsw_search_batch_diverse calls answered),
 * "diverse_launches" (selections launched, hnsw_diversify_device's included).
 * Not provided: compile-time-dimension distance routines inside the selection (it runs the any-dimension routine);
 * a lambda per query; MMR over shards (merged lists carry global ids); one-query gathered calls; the Rust shim's
 * binding. */
#define HNSW_DIVERSE_POOL_MAX 256
int hnsw_diversify_device(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_out, float lambda,
                          const uint32_t *d_ids_in /* nq x pool */, const float *d_dists_in,
                          const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                          uint32_t *d_ids, float *d_dists /* nq x n_out */, float *d_gaps /* or NULL */,
                          uint32_t *d_counts /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                          void *stream);
int hnsw_search_batch_diverse(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef,
                              float lambda, hnsw_mask_set *set /* or NULL */, const uint32_t *mask_of /* nq, or NULL */,
                              const uint32_t *lo, const uint32_t *hi /* nq each, or both NULL: no range */,
                              uint32_t *ids /* nq x n */, float *dists /* or NULL */, float *gaps /* or NULL */,
                              uint32_t *counts /* or NULL */, hnsw_query_stats *stats /* or NULL */);

/* ---- search from stored rows: queries by id and by weighted ids -------------------------------------------------------
 * An extension (the reference searches by vector only): "nearest to this item I already stored" -- more like this,
 * recommendation from liked and disliked items, the centroid of a few stored rows, the k-NN graph of the whole index,
 * a near-duplicate sweep.  The rows are in HBM next to the graph, so the query rows are made there and the sources are
 * taken back out of the result lists there; a replica handle, which has no host rows, serves as well.
 * A call has nq queries of `width` slots each, 1 <= width <= HNSW_FROM_ROWS_MAX_TERMS: src_ids [nq][width], a slot
 * holding UINT32_MAX is absent (pads may sit anywhere), and weights [nq][width] f32, NULL: every weight is 1.0f.
 * THE ROW of an id is exactly what hnsw_get_vector returns: the stored bits (f32 kind), ((float)code * delta) + min, two
 * separately rounded operations (8-bit kind); under the metric_cosine option the stored unit row.
 * THE COMPOSED QUERY: element e of query q is folded over the present slots in slot order, acc = w * x for the first
 * present slot and acc = acc + (w * x) for every later one: plain f32 operations, never fused, so numpy float32
 * restates them.  Starting from the first product keeps a -0 element -0; with width = 1 and no weights the row is bit
 * for bit hnsw_get_vector's.  A NaN or infinite weight is no argument error: it makes a NaN query, and that query gets
 * the search's own HNSW_ERR_NAN_INPUT.  The bit pattern of a NaN element is not part of the contract.
 * THE COMPOSE STATUS (int32 per query) is HNSW_ERR_ARG when the query has no present slot or a present id at or beyond
 * the index length, else HNSW_OK.  For a failed query no stored row is read (the check precedes the first read) and its
 * output row is all zeros.  Every output word is written exactly once.
 * THE DROP out of one query's candidate list (id_j, dist_j), j < n_in, with an exclusion list ex [width] (UINT32_MAX:
 * absent) and output length n_out:
 *   - entry j is PRESENT iff j < min(count, n_in), or, without counts, iff id_j != UINT32_MAX; a query whose incoming
 *     status is not HNSW_OK has no present entry; nor has a query whose optional compose status (src_status) is not
 *     HNSW_OK, and its stats record then carries that status (it takes precedence over the incoming one);
 *   - the output is the present entries whose id equals no present exclusion id, in input order, cut to the first n_out,
 *     with the input's distance bits; ids are padded with UINT32_MAX and dists with +inf; counts = the number written;
 *   - dropped (optional) = the present entries removed by the exclusion over all n_in; an entry listed twice counts
 *     twice.  An absent exclusion slot never matches an absent entry.  Nothing is sorted;
 *   - the stats record passes through otherwise unchanged.
 * Limits: 1 <= n_out <= n_in <= HNSW_DROP_MAX_N (the register-resident list, as HNSW_RADIUS_MAX_N).
 *
 * hnsw_compose_rows_device writes THE COMPOSED QUERY of nq queries to d_Q [nq][dim] and THE COMPOSE STATUS to d_status
 * [nq] (or NULL); every d_* pointer is device memory.  It reads the snapshot only, so a replica handle serves.  After
 * the snapshot is brought up to date ONE launch (the distance seam's kernel in its compose form, one wave per query) is
 * enqueued on `stream`; nothing is allocated, copied or synchronised on it.  HNSW_ERR_ARG, decided before the device is
 * touched: h NULL; width outside its limits; nq > 2^31 - 1; d_src_ids or d_Q NULL.  nq == 0 is HNSW_OK on any handle and
 * launches nothing; an empty index is HNSW_ERR_EMPTY.
 * hnsw_drop_ids_device is THE DROP alone over lists in HBM (no handle, as hnsw_radius_cut_device): the inputs are what
 * any *_device search leaves after its _finish, d_ex [nq][width] the exclusion ids, d_src_status [nq] or NULL.  ONE
 * launch (the exact path's merge kernel in its drop form, one wave per query) is enqueued on `stream`; nothing is
 * allocated, copied or synchronised.  Outputs must not overlap inputs.  d_counts and d_dropped may be NULL; d_stats is
 * required iff d_stats_in is given.  HNSW_ERR_ARG, decided before the device is touched: the limits violated; width
 * outside its limits; nq > 2^31 - 1; d_ex, d_ids_in, d_dists_in, d_ids or d_dists NULL; exactly one of d_stats_in /
 * d_stats given.  nq == 0 is HNSW_OK and launches nothing.
 * With these two and the *_device searches (the filtered ones included) a caller chains compose, search and drop
 * without leaving HBM; inside the capture conditions of hnsw_search_batch_device the three launches are one chain of a
 * captured graph.
 *
 * hnsw_search_batch_from_rows: with exclude != 0 the result is THE DROP, with the sources as exclusion list and n_out =
 * n, of what hnsw_search_batch returns for the composed queries with n' = n + width, on the same handle with the same
 * options; with exclude == 0 it is that call with n' = n and no drop is launched.  Everything of the candidate call is
 * inherited: the cosine option applied to the composed query, the counters, count < n when ef is small, deletions,
 * per-query errors (the first is returned, every other row is filled in).  The walk uses the QUERY-side arithmetic, as
 * any query does: an 8-bit row is re-quantised as a query, so distances are not promised to equal hnsw_distance(src,
 * hit) for that kind.  A deleted source is a legal source: its row is still stored, and no search returns it.  Limits:
 * n >= 1 and n + width <= HNSW_DROP_MAX_N.  All arrays are the host's, so a present source id at or beyond the index
 * length, or a query without a present slot, fails the WHOLE call with HNSW_ERR_ARG (the message names the query) before
 * the device is touched.  With nothing deleted the call stays on the device: ids and weights go up once, one compose
 * launch, hnsw_search_batch_device and its _finish on the composed rows, one drop launch, one copy of the result block
 * back.  While ids are deleted the candidates are the HOST form's (the composed rows are copied back, hnsw_search_batch
 * runs on them, its lists go up before the drop) and n + width <= 64 is required.  dists, counts and stats may be NULL.
 * hnsw_search_batch_by_id is the same call with width = 1 and no weights.  nq == 0 is HNSW_OK; an empty index is
 * HNSW_ERR_EMPTY.  hnsw_get_stat: "from_rows_calls" (calls answered), "from_rows_compose_launches"
 * (hnsw_compose_rows_device's included), "from_rows_drop_launches" (those of the two search calls; hnsw_drop_ids_device
 * takes no handle to count on).
 * Not provided: a label range or mask row in the host entry point (the primitives compose with the filtered *_device
 * entries); stored-against-stored arithmetic in the walk; one-query gathered calls; the Rust shim's binding. */
#define HNSW_FROM_ROWS_MAX_TERMS 64
#define HNSW_DROP_MAX_N 1024
int hnsw_compose_rows_device(hnsw_index *h, uint64_t nq, uint32_t width, const uint32_t *d_src_ids /* nq x width */,
                             const float *d_weights /* nq x width, or NULL */, float *d_Q /* nq x dim */,
                             int32_t *d_status /* nq, or NULL */, void *stream);
int hnsw_drop_ids_device(uint64_t nq, uint32_t n_in, uint32_t n_out, uint32_t width,
                         const uint32_t *d_ex /* nq x width */, const int32_t *d_src_status /* nq, or NULL */,
                         const uint32_t *d_ids_in, const float *d_dists_in /* nq x n_in */,
                         const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                         uint32_t *d_ids, float *d_dists /* nq x n_out */, uint32_t *d_counts /* or NULL */,
                         uint32_t *d_dropped /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                         void *stream);
int hnsw_search_batch_from_rows(hnsw_index *h, const uint32_t *src_ids /* nq x width */,
                                const float *weights /* nq x width, or NULL */, uint64_t nq, uint32_t width, uint32_t n,
                                uint32_t ef, int exclude, uint32_t *ids /* nq x n */, float *dists /* or NULL */,
                                uint32_t *counts /* or NULL */, hnsw_query_stats *stats /* or NULL */);
int hnsw_search_batch_by_id(hnsw_index *h, const uint32_t *src_ids /* nq */, uint64_t nq, uint32_t n, uint32_t ef,
                            int exclude_self, uint32_t *ids /* nq x n */, float *dists /* or NULL */,
                            uint32_t *counts /* or NULL */, hnsw_query_stats *stats /* or NULL */);

/* ---- multi-vector search: several vectors per query, their result lists fused on the device ---------------------------
 * An extension (the reference takes one vector per query): a text and an image embedding of one request, three rewrites
 * of one question, "near any of these examples" -- Weaviate's multi-target vectors (sum / min / manual weights), Qdrant's
 * multi-query, Milvus's weighted hybrid search.  This is not the composed query of the block above: a centroid's
 * neighbours are not the points with the smallest summed distance to the parts, and "nearest to any of them" has no
 * composed form.
 * A call has nq queries of T = n_vecs vectors each: Q [nq][T][dim], weights [nq][T] f32 (NULL: every weight 1.0f and no
 * multiply), candidate ids ids_in [nq][T][pool], counts_in [nq][T] or NULL, stats_in [nq][T] or NULL.  Limits: 1 <= T <=
 * HNSW_MULTI_MAX_VECS, 1 <= n_out <= pool, T * pool <= HNSW_FUSE_MAX_CANDS.  mode is HNSW_FUSE_SUM or HNSW_FUSE_MIN.
 * THE FUSION of one query:
 *   - entry j of list t is PRESENT iff j < min(counts_in[t], pool), or, without counts, iff its id is not UINT32_MAX.  If
 *     any of the query's T incoming statuses is not HNSW_OK the query has no present entry: its status is the first one
 *     that is not HNSW_OK in vector order, its count 0 and its rows padded;
 *   - a present id at or beyond the index length gives the query HNSW_ERR_ARG, count 0 and padded rows, and no stored row
 *     is read for it;
 *   - a vector with a NaN element gives the query HNSW_ERR_NAN_INPUT, count 0 and padded rows.  Precedence: the incoming
 *     status, then HNSW_ERR_ARG, then HNSW_ERR_NAN_INPUT;
 *   - the candidate set C is the DISTINCT present ids over all T lists: an id listed several times, inside one list or
 *     across lists, is one candidate; unique = |C| (0 for a failed query);
 *   - D_t(c), for every t < T and every c in C whether or not list t holds c, is the bits of hnsw_distance_batch(h, q_t,
 *     {c}): the query-side arithmetic (an 8-bit query is quantised as any query is; under the metric_cosine option the
 *     vector is normalised once from the caller's raw row).  The lists' own distances are not an input;
 *   - the fold, with p_t = w_t * D_t(c) one f32 multiply (omitted when weights is NULL).  HNSW_FUSE_SUM: s = p_0, then
 *     s = s + p_t for t = 1 .. T-1 in vector order, each operation rounded separately and never contracted.
 *     HNSW_FUSE_MIN: s = +inf, then s = p_t < s ? p_t : s in vector order (a NaN term leaves s as it is).  Negative and
 *     zero weights are legal; a NaN or infinite weight is no argument error;
 *   - a candidate whose score is NaN is never returned; the others are ranked by (score under f32 <, -0 == +0; then id
 *     ascending), so the answer depends neither on the order of the lists nor on which duplicate was kept.
 * Per query: ids [n_out] (pad UINT32_MAX), scores [n_out] (the fold's own bits, pad +inf), counts = entries written,
 * unique (optional), stats (optional): n_dist, n_exp and sum_deg the wrapping uint32 sums of the T incoming records (the
 * fusion's own evaluations are not counted), the status as above.  Every output word is written exactly once.
 * The answer is the best n_out of the UNION of the per-vector pools, not of the whole index: a point that is in no
 * vector's pool is not a candidate, however small its summed distance.  A caller who wants more raises `pool`.
 *
 * hnsw_fuse_lists_device is THE FUSION alone over buffers in HBM: every d_* pointer is device memory, the lists are what
 * any *_device search of the same handle leaves after its _finish for the nq * T rows of d_Q taken as one batch (ids
 * local to the handle, so a replica handle serves).  After the snapshot is brought up to date ONE launch (the distance
 * seam's kernel in its fusion form, one wave per query) is enqueued on `stream` and the call returns without
 * synchronising it.  Under the metric_cosine option it reads a stream-ordered unit-length copy of d_Q, exactly as
 * hnsw_search_batch_device does; otherwise nothing is allocated or copied, and the call is capturable under that call's
 * conditions.  The status of a failed query is written to d_stats only (the call cannot see it).  Outputs must not
 * overlap inputs.  d_weights, d_counts_in, d_counts and d_unique may be NULL; d_stats is required iff d_stats_in is
 * given.  HNSW_ERR_ARG, decided before the device is touched: h NULL; the limits violated; a mode other than the two;
 * nq > 2^31 - 1; d_Q, d_ids_in, d_ids or d_scores NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK on
 * any handle, whatever else is passed, and launches nothing; an empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_multi answers host-pointer queries of T vectors each by their n best.  By definition the result is
 * THE FUSION, with n_out = n, of the lists that hnsw_search_batch returns for the nq * T rows of Q taken as one batch
 * with n = pool and ef' = max(ef, pool, 1), on the same handle with the same options.  Everything of that call is
 * inherited: deletions, the cosine option, per-query errors (the first is returned with the QUERY named, not the row;
 * every other row is filled in).  With nothing deleted the call stays on the device: Q and the weights go up once (the
 * cosine option's unit copy made once, for the search and the fusion), the launch of hnsw_search_batch_device and the
 * re-run loop of its _finish over nq * T queries, one fusion launch, ONE copy of the block [ids | scores | counts | unique | stats] back.  While ids are deleted the candidates are the host
 * form's and go up before the fusion; pool <= 64 is then required.  scores, counts, unique and stats may be NULL.
 * HNSW_ERR_ARG, decided before the device is touched: the limits violated; a mode other than the two; Q or ids NULL;
 * nq * T > 2^31 - 1.  nq == 0 is HNSW_OK; an empty index is HNSW_ERR_EMPTY.  hnsw_get_stat: "multi_calls"
 * (hnsw_search_batch_multi calls answered), "multi_fuse_launches" (fusions launched, hnsw_fuse_lists_device's included).
 * Not provided: per-hit per-vector distances; a different T per query; filters other than deletions in the host entry
 * (the primitive chains with the filtered *_device searches); rank fusion (see "hybrid search" below:
 * hnsw_fuse_ranked_device); fusion over shards (merged lists carry global
 * ids); one-query gathered calls; the Rust shim's binding. */
#define HNSW_MULTI_MAX_VECS 16
#define HNSW_FUSE_MAX_CANDS 256
#define HNSW_FUSE_SUM 0
#define HNSW_FUSE_MIN 1
int hnsw_fuse_lists_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                           const float *d_Q /* nq x n_vecs x dim */, const float *d_weights /* nq x n_vecs, or NULL */,
                           const uint32_t *d_ids_in /* nq x n_vecs x pool */, const uint32_t *d_counts_in /* or NULL */,
                           const hnsw_query_stats *d_stats_in /* or NULL */, uint32_t *d_ids, float *d_scores /* nq x n_out */,
                           uint32_t *d_counts /* or NULL */, uint32_t *d_unique /* or NULL */,
                           hnsw_query_stats *d_stats /* required iff d_stats_in */, void *stream);
int hnsw_search_batch_multi(hnsw_index *h, const float *Q /* nq x n_vecs x dim */, uint64_t nq, uint32_t n_vecs,
                            const float *weights /* nq x n_vecs, or NULL */, uint32_t mode, uint32_t n, uint32_t pool,
                            uint32_t ef, uint32_t *ids /* nq x n */, float *scores /* or NULL */,
                            uint32_t *counts /* or NULL */, uint32_t *unique /* or NULL */,
                            hnsw_query_stats *stats /* or NULL */);

/* ---- late-interaction search: documents of several rows scored by summed min distance, on the device -------------------
 * An extension (the reference scores rows, one vector per query): the way multi-vector retrieval models (ColBERT,
 * ColPali and their kin) are served.  A document is the rows that share a label (hnsw_set_labels); a query of T vectors
 * is scored against it by taking, for every query vector, the distance to the document's nearest row, and adding those up
 * (MaxSim / Chamfer).  Neither hnsw_search_batch_multi (it scores rows: the row with the smallest summed distance to all
 * vectors is not the document whose rows cover the vectors best) nor hnsw_search_batch_grouped (it collapses one list by
 * rank and never looks at a second vector) answers this.
 * A call has nq queries of T = n_vecs vectors each: Q [nq][T][dim], candidate ids ids_in [nq][T][pool], counts_in [nq][T]
 * or NULL, stats_in [nq][T] or NULL.  Limits: 1 <= T <= HNSW_LATE_MAX_VECS, T * pool <= HNSW_LATE_MAX_CANDS, 1 <= n_out
 * <= min(T * pool, HNSW_LATE_MAX_DOCS).  mode is HNSW_LATE_SUM or HNSW_LATE_SUM_SQ.
 * THE LATE INTERACTION of one query:
 *   - presence, the incoming statuses, the range and NaN vectors are THE FUSION's rules, word for word: entry j of list t
 *     is PRESENT iff j < min(counts_in[t], pool), or, without counts, iff its id is not UINT32_MAX; the first incoming
 *     status that is not HNSW_OK fails the query with that status; otherwise a present id at or beyond the index length
 *     gives HNSW_ERR_ARG, and no stored row is read for the query; otherwise a NaN element in any vector gives
 *     HNSW_ERR_NAN_INPUT.  A failed query has count 0, n_docs 0 and padded rows;
 *   - the candidate set C is the DISTINCT present ids over all T lists;
 *   - lab(c) is the handle's label of c as of the call: 0 at or beyond the column's length, and 0 everywhere on a handle
 *     that never had a label set (which makes one document);
 *   - the documents are the distinct labels over C; n_docs is their number, doc_size(g) the number of c in C with
 *     lab(c) == g;
 *   - D_t(c), for every t < T and every c in C, is the bits of hnsw_distance_batch(h, q_t, {c}), as in THE FUSION (an 8-bit
 *     query is quantised as any query is; under the metric_cosine option the vector is normalised once from the caller's
 *     raw row).  The lists' own distances are not an input;
 *   - the per-vector minimum m_t(g) starts at +inf and becomes D_t(c) wherever D_t(c) < m_t(g) under f32 <, over the c of
 *     document g (a NaN leaves it as it is): a minimum, so the order of the c does not matter;
 *   - the fold: e_t = m_t(g) under HNSW_LATE_SUM, e_t = m_t(g) * m_t(g), one f32 multiply, under HNSW_LATE_SUM_SQ; s = e_0,
 *     then s = s + e_t for t = 1 .. T-1 in vector order, each operation rounded separately and never contracted.  On
 *     unit-length rows (what the cosine option gives) SUM_SQ is 2T - 2 * sum_t max_c cos(q_t, c): exactly MaxSim's
 *     ranking.  SUM is the Chamfer distance in the index's own metric;
 *   - best(g) is the c of document g with the smallest (bits of D_t(c), c) over all t and all c of g, NaN distances left
 *     out; UINT32_MAX if there is none.  It is the row a caller shows as the hit;
 *   - a document whose score is NaN is never returned; the others are ranked by (score under f32 <, -0 == +0; then label
 *     ascending).
 * Per query: doc_labels [n_out] (pad 0), scores [n_out] (the fold's own bits, pad +inf), best_ids [n_out] (optional, pad
 * UINT32_MAX), doc_sizes [n_out] (optional, pad 0), counts (optional) = entries written, n_docs (optional), stats
 * (required iff stats_in is given): n_dist, n_exp and sum_deg the wrapping uint32 sums of the T incoming records, the
 * status as above.  Every output word is written exactly once.
 * The documents scored are those with a row in some vector's pool, and a document's minimum runs over its rows IN C, not
 * over all its stored rows: a row that is in no vector's pool does not lower its document's score, however near it is.
 * A caller who wants more raises `pool`.
 *
 * hnsw_late_interaction_device is THE LATE INTERACTION alone over buffers in HBM, exactly as hnsw_fuse_lists_device is THE
 * FUSION: the snapshot is brought up to date, the label column's HBM copy as hnsw_group_by_label_device does it; under the
 * metric_cosine option a stream-ordered unit-length copy of d_Q is made; then ONE launch (the distance seam's kernel in
 * its late-interaction form, one wave per query) is enqueued on `stream`, which is not synchronised.  Outputs must not
 * overlap inputs.  The status of a failed query is written to d_stats only.  HNSW_ERR_ARG, decided before the device is
 * touched: h NULL; a limit violated; a mode other than the two; nq > 2^31 - 1; d_Q, d_ids_in, d_doc_labels or d_scores
 * NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK on any handle, whatever else is passed, and
 * launches nothing; an empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_late answers host-pointer queries of T vectors each by their n best documents.  By definition the
 * result is THE LATE INTERACTION, with n_out = n, of the lists that hnsw_search_batch returns for the nq * T rows of Q
 * taken as one batch with n = pool and ef' = max(ef, pool, 1), on the same handle with the same options.  With nothing
 * deleted the call stays on the device: Q goes up once (the cosine option's unit copy made once, for the search and the
 * late interaction), the launch of hnsw_search_batch_device and the re-run loop of its _finish over nq * T queries, one
 * late-interaction launch, ONE copy of the block [labels | scores | best ids | sizes | counts | n_docs | stats] back.
 * While ids are deleted the candidates are the host form's and go up before the launch; pool <= 64 is then required.
 * Per-query errors are inherited: the first is returned with the QUERY named, not the row, and every other row is filled
 * in.  scores, best_ids, doc_sizes, counts, n_docs and stats may be NULL.  HNSW_ERR_ARG, decided before the device is
 * touched: the limits violated; a mode other than the two; Q or doc_labels NULL; nq * T > 2^31 - 1.  nq == 0 is HNSW_OK;
 * an empty index is HNSW_ERR_EMPTY.  hnsw_get_stat: "late_calls" (hnsw_search_batch_late calls answered), "late_launches"
 * (late interactions launched, hnsw_late_interaction_device's included).
 * Completing a document with its rows that are in no pool is hnsw_search_batch_late_exact ("exact document scoring").
 * Not provided: a different T per query, or a mask over a query's vectors; weights per vector; filters other than
 * deletions in the host entry (the primitive chains with the filtered *_device searches); late interaction over shards;
 * one-query gathered calls; the Rust shim's binding. */
#define HNSW_LATE_MAX_VECS 32
#define HNSW_LATE_MAX_CANDS 1024
#define HNSW_LATE_MAX_DOCS 256
#define HNSW_LATE_SUM 0
#define HNSW_LATE_SUM_SQ 1
int hnsw_late_interaction_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                                 const float *d_Q /* nq x n_vecs x dim */, const uint32_t *d_ids_in /* nq x n_vecs x pool */,
                                 const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                                 uint32_t *d_doc_labels, float *d_scores /* nq x n_out */, uint32_t *d_best_ids /* or NULL */,
                                 uint32_t *d_doc_sizes /* or NULL */, uint32_t *d_counts /* or NULL */,
                                 uint32_t *d_n_docs /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                                 void *stream);
int hnsw_search_batch_late(hnsw_index *h, const float *Q /* nq x n_vecs x dim */, uint64_t nq, uint32_t n_vecs, uint32_t mode,
                           uint32_t n, uint32_t pool, uint32_t ef, uint32_t *doc_labels /* nq x n */,
                           float *scores /* or NULL */, uint32_t *best_ids /* or NULL */, uint32_t *doc_sizes /* or NULL */,
                           uint32_t *counts /* or NULL */, uint32_t *n_docs /* or NULL */,
                           hnsw_query_stats *stats /* or NULL */);

/* ---- exact document scoring: late interaction over every stored row ------------------------------------------------------
 * An extension, and the stage late-interaction search leaves open: there a document's minimum runs over its rows that
 * landed in some vector's pool.  Here the documents a list names are scored over EVERY stored row they have, the way
 * ColBERT-style serving (PLAID's last stage) completes its approximate candidates -- and the way documents that come from
 * elsewhere (a lexical retriever, a grouped search) are scored against a multi-vector query.
 * A call has nq queries of T = n_vecs vectors each: Q [nq][T][dim], ONE list of document labels docs_in [nq][n_in],
 * counts_in [nq] or NULL, stats_in [nq] or NULL.  Limits: 1 <= T <= HNSW_LATE_MAX_VECS, 1 <= n_out <= n_in <=
 * HNSW_DOCS_MAX_IN, 1 <= rows_cap <= HNSW_DOCS_MAX_ROWS (the kernel keeps the running totals of the scored rows as 32-bit
 * words: HNSW_DOCS_MAX_IN documents of HNSW_DOCS_MAX_ROWS rows are 2^28).  mode is HNSW_LATE_SUM or HNSW_LATE_SUM_SQ.
 * THE DOCUMENT SCORING of one query:
 *   - entry j of the list is PRESENT iff j < min(counts_in, n_in); without counts every one of the n_in entries is present:
 *     every uint32 is a label, so there is no pad value.  Duplicate labels in a list are one document;
 *   - an incoming status that is not HNSW_OK fails the query with that status; otherwise a NaN element in any vector gives
 *     HNSW_ERR_NAN_INPUT.  A failed query has count 0, n_docs 0 and padded rows, and no stored row is read for it;
 *   - R(g), the rows of label g, is the ids below hnsw_len that are not deleted and whose label is g as of the call: the
 *     label is 0 at or beyond the column's length, and 0 everywhere on a handle that never had a label set.
 *     doc_size(g) = |R(g)|.  A label with doc_size 0 is not a document: it is dropped and not counted in n_docs;
 *   - the rows scored are the min(doc_size(g), rows_cap) lowest ids of R(g); doc_sizes reports the full doc_size(g), so a
 *     caller sees that a document was cut;
 *   - D_t(c), m_t(g), the fold, best(g) and the order are THE LATE INTERACTION's, word for word, with one change: the
 *     minimum, and best(g), run over the rows scored instead of the candidates of g.
 * Outputs and pads are THE LATE INTERACTION's: doc_labels [n_out] (pad 0), scores [n_out] (pad +inf), best_ids [n_out]
 * (optional, pad UINT32_MAX), doc_sizes [n_out] (optional, pad 0), counts (optional), n_docs (optional), stats (required
 * iff stats_in is given): the incoming record with the status as above.  Every output word is written exactly once.
 *
 * hnsw_score_documents_device is THE DOCUMENT SCORING alone over buffers in HBM, under the stream contract of
 * hnsw_late_interaction_device: the snapshot is brought up to date; under the metric_cosine option a stream-ordered
 * unit-length copy of d_Q is made; the DOCUMENT INDEX -- the keys label << 32 | id of the undeleted ids, ascending, 8 bytes
 * each in HBM -- is brought up to date on a stream of the handle's own, which is synchronised: one whole copy when the
 * labels, the deleted set or the length changed since it was made, nothing otherwise; then ONE launch (the distance seam's
 * kernel in its document-scoring form, one wave per query) is enqueued on `stream`, which is not synchronised.  The index is
 * derived from the label column and the deleted set: it is not saved and no part of the snapshot exchange, and hnsw_clone
 * and hnsw_set_device make it afresh on first use.  Outputs must not overlap inputs.  The status of a failed query is
 * written to d_stats only.  HNSW_ERR_ARG, decided before the device is touched: h NULL; a limit violated; a mode other
 * than the two; nq > 2^31 - 1; d_Q, d_docs_in, d_doc_labels or d_scores NULL; exactly one of d_stats_in / d_stats given.
 * nq == 0 is HNSW_OK on any handle, whatever else is passed, and launches nothing; an empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_late_exact answers host-pointer queries of T vectors each by their n best documents, every returned
 * document scored over all its rows.  By definition the result is THE DOCUMENT SCORING, with n_out = n, of the labels,
 * counts and stats that THE LATE INTERACTION returns with n_out = n_cand over the lists of hnsw_search_batch_late's own
 * candidate call (n = pool, ef' = max(ef, pool, 1)).  Limits: T * pool <= HNSW_LATE_MAX_CANDS, 1 <= n <= n_cand <=
 * min(T * pool, HNSW_DOCS_MAX_IN).  Q goes up once, then the search and its re-run loop, one late-interaction launch, one
 * scoring launch, ONE copy of the block [labels | scores | best ids | sizes | counts | n_docs | stats] back.  While ids are
 * deleted the candidates are the host form's, as in hnsw_search_batch_late; pool <= 64 is then required.  Per-query errors
 * and the optional outputs are hnsw_search_batch_late's.  nq == 0 is HNSW_OK; an empty index is HNSW_ERR_EMPTY.
 * hnsw_get_stat: "docs_calls" (hnsw_search_batch_late_exact calls answered), "docs_launches" (scorings launched,
 * hnsw_score_documents_device's included; the composed call also counts its late interaction in "late_launches"),
 * "doc_index_uploads" and "doc_index_keys_uploaded" (whole copies of the document index, and the keys they carried).
 * Not provided: incremental maintenance of the document index; a different T per query; weights per vector; scoring over
 * shards; filters other than deletions in the host entry; one-query gathered calls; the Rust shim's binding. */
#define HNSW_DOCS_MAX_IN 256
#define HNSW_DOCS_MAX_ROWS 1048576
int hnsw_score_documents_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t n_in, uint32_t n_out, uint32_t rows_cap,
                                uint32_t mode, const float *d_Q /* nq x n_vecs x dim */,
                                const uint32_t *d_docs_in /* nq x n_in labels */, const uint32_t *d_counts_in /* nq, or NULL */,
                                const hnsw_query_stats *d_stats_in /* nq, or NULL */, uint32_t *d_doc_labels,
                                float *d_scores /* nq x n_out */, uint32_t *d_best_ids /* or NULL */,
                                uint32_t *d_doc_sizes /* or NULL */, uint32_t *d_counts /* or NULL */,
                                uint32_t *d_n_docs /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */,
                                void *stream);
int hnsw_search_batch_late_exact(hnsw_index *h, const float *Q /* nq x n_vecs x dim */, uint64_t nq, uint32_t n_vecs,
                                 uint32_t mode, uint32_t n, uint32_t n_cand, uint32_t rows_cap, uint32_t pool, uint32_t ef,
                                 uint32_t *doc_labels /* nq x n */, float *scores /* or NULL */, uint32_t *best_ids /* or NULL */,
                                 uint32_t *doc_sizes /* or NULL */, uint32_t *counts /* or NULL */,
                                 uint32_t *n_docs /* or NULL */, hnsw_query_stats *stats /* or NULL */);

/* ---- refined search: the pool re-scored against full rows kept in HBM ------------------------------------------------
 * An extension (the reference ranks by the rows it stores).  Every search above ranks by the distance the INDEX stores:
 * its 8-bit rows, or its f32 rows of the index's own dimension.  A caller who also holds a better representation of the
 * same ids -- the full 768-d embedding while the index was built over the first 128 coordinates (Matryoshka-style
 * "funnel" retrieval), full-precision rows behind the 8-bit kind, any second-stage vector -- keeps it in a ROW TABLE in
 * HBM, and a search is answered by a walk over the index's short rows followed by an exact re-score of a small pool
 * against the long ones.
 *
 * A row table (hnsw_row_table) is rows x full_dim elements of dtype HNSW_ROWS_F32 or HNSW_ROWS_F16 (IEEE binary16,
 * widened exactly to f32 where it is read), row id = index id, 1 <= full_dim <= HNSW_REFINE_MAX_DIM.  It lives in HBM
 * ONLY, on its handle's device: the host keeps no copy, the caller owns the full rows.  It is NOT saved by hnsw_save, NOT
 * cloned by hnsw_clone and NOT part of the snapshot exchange.
 *   hnsw_row_table_create   touches no device; the first write allocates on the handle's device (its snapshot's, else the
 *                           one it is bound to, else the calling thread's) and fixes it.
 *   hnsw_row_table_write    n rows of f32 to ids first_id .. first_id + n - 1.  An f16 table rounds to nearest, ties to
 *                           even, on the host.  A NaN, an infinity or a value that rounds to one is HNSW_ERR_NAN_INPUT and
 *                           nothing is written.  first_id <= rows: there are no holes (HNSW_ERR_ARG).  A write past the
 *                           capacity grows the array by a device-to-device copy (capacity + 1/8).
 *   hnsw_row_table_write_raw  the same with rows in the table's own dtype; every element must be finite.
 *   hnsw_row_table_read     rows back as f32, widened exactly.
 *   hnsw_row_table_device   the array in HBM (NULL before the first write) and its rows, for hnsw_refine_device.  A later
 *                           write that grows the table moves it.
 *   hnsw_f32_to_f16         the rounding routine itself, device-free: HNSW_ERR_NAN_INPUT, and nothing written, when a
 *                           value is a NaN or rounds to an infinity (65520 is the first that does).
 * Writes to one table are serialised; a write must not run while a search names the table.
 *
 * THE REFINEMENT of one query, with a candidate list ids_in [pool], counts_in or NULL, stats_in or NULL, a full query row
 * qf [full_dim] of f32 and a table of table_rows rows:
 *   - entry j is PRESENT iff j < min(count, pool), or, without counts, iff its id is not UINT32_MAX (THE SELECTION's rule);
 *   - an incoming status that is not HNSW_OK fails the query with that status; otherwise a present id at or beyond
 *     table_rows gives HNSW_ERR_ARG, and no table row is read for the query; otherwise a NaN element of qf gives
 *     HNSW_ERR_NAN_INPUT.  A failed query has count 0 and padded rows;
 *   - the distance of a present entry with row x is sqrt(s), where s = 0.0f, then t = x[e] - qf[e]; s = s + t * t for
 *     e = 0 .. full_dim - 1: ONE left-to-right f32 chain, every operation rounded separately and never contracted, the
 *     correctly rounded square root -- FullVec::distance's own arithmetic (vectors/src/full.rs:23-29).  An f16 element is
 *     widened exactly before the subtraction: subnormals, +-0 and 65504 survive;
 *   - the present entries are ranked ascending by (distance bits, id); duplicate ids in a list are separate entries; an
 *     entry whose distance is +inf is an ordinary entry and ranks last; one whose distance is NaN is never returned.
 * Per query: ids [n_out] (pad UINT32_MAX), dists [n_out] (pad +inf), counts (optional) = entries written, stats (required
 * iff stats_in is given): the incoming record unchanged but for the status above.  Every output word is written exactly
 * once.  Limits: 1 <= n_out <= pool <= HNSW_REFINE_POOL_MAX, 1 <= full_dim <= HNSW_REFINE_MAX_DIM, nq <= 2^31 - 1.
 *
 * hnsw_refine_device is THE REFINEMENT alone over buffers in HBM.  It takes no handle, as hnsw_merge_topk_device and
 * hnsw_radius_cut_device take none: ONE launch (the distance seam's kernel in its refinement form, one wave per query) is
 * enqueued on `stream` -- no synchronise, no allocation, no copy.  d_table holds table_rows x full_dim elements of dtype,
 * d_Qfull nq x full_dim floats; outputs must not overlap inputs.  The status of a failed query is written to d_stats
 * only.  HNSW_ERR_ARG, decided before the device is touched: a limit violated; a dtype other than the two; nq > 2^31 - 1;
 * d_table, d_Qfull, d_ids_in, d_ids or d_dists NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK
 * whatever else is passed.
 *
 * hnsw_search_batch_refined answers host-pointer queries.  By definition the result is THE REFINEMENT, with n_out = n
 * and the rows of Qfull, of the lists that the candidate call of hnsw_search_batch_diverse's table returns for Q with
 * n = pool and ef' = max(ef, pool, 1), and everything is inherited exactly as there: the filter (set / mask_of / lo / hi),
 * deleted ids taken out, the planner, per-query errors, pool <= 64 and ef' <= 256 under a filter or deletions.  The
 * metric_cosine option applies to Q alone; Qfull is used as given.  Q == NULL: the index's queries are the first dim
 * elements of each Qfull row (full_dim >= dim is then required), taken by one strided upload.  Unfiltered and with nothing
 * deleted the call stays on the device: both query blocks go up once, the launch of hnsw_search_batch_device and the
 * re-run loop of its _finish, one refinement launch, ONE copy of the block [ids | dists | counts | stats] back.  dists,
 * counts and stats may be NULL.  HNSW_ERR_ARG, decided before the device is touched: the filter's own refusals; t NULL or
 * of another handle; a limit violated; Qfull or ids NULL; nq > 2^31 - 1; Q NULL with full_dim < dim; a table with fewer
 * rows than the index.  nq == 0 is HNSW_OK; an empty index is HNSW_ERR_EMPTY.  hnsw_get_stat: "refine_calls"
 * (hnsw_search_batch_refined calls answered), "refine_launches" (the refinements they launched), "row_table_writes"
 * (writes that reached a table of the handle).
 * Not provided: bf16 rows; a table per shard and a refined partitioned search; the table inside hnsw_save (hnsw_row_table_save, below, writes it to a file of its own); one-query
 * gathered calls; the Rust shim's binding; a place in the update machine (an inserted id needs its full row written
 * before a search may return it: the table must cover the index). */
#define HNSW_ROWS_F32 0
#define HNSW_ROWS_F16 1
#define HNSW_REFINE_POOL_MAX 1024
#define HNSW_REFINE_MAX_DIM 4096
typedef struct hnsw_row_table hnsw_row_table;
int hnsw_row_table_create(hnsw_index *h, uint32_t full_dim, uint32_t dtype, hnsw_row_table **out);
void hnsw_row_table_free(hnsw_row_table *t);
int hnsw_row_table_info(const hnsw_row_table *t, uint32_t *full_dim, uint32_t *dtype, uint64_t *rows);
int hnsw_row_table_write(hnsw_row_table *t, uint64_t first_id, uint64_t n, const float *rows /* n x full_dim */);
int hnsw_row_table_write_raw(hnsw_row_table *t, uint64_t first_id, uint64_t n, const void *rows /* in the table's dtype */);
int hnsw_row_table_read(hnsw_row_table *t, uint64_t first_id, uint64_t n, float *out /* n x full_dim */);
int hnsw_row_table_device(const hnsw_row_table *t, const void **d_ptr, uint64_t *rows /* or NULL */);
int hnsw_f32_to_f16(const float *in, uint64_t n, uint16_t *out);
int hnsw_refine_device(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t full_dim, uint32_t dtype,
                       const void *d_table /* table_rows x full_dim of dtype */, uint64_t table_rows,
                       const float *d_Qfull /* nq x full_dim */, const uint32_t *d_ids_in /* nq x pool */,
                       const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                       uint32_t *d_ids, float *d_dists /* nq x n_out */, uint32_t *d_counts /* or NULL */,
                       hnsw_query_stats *d_stats /* required iff d_stats_in */, void *stream);
int hnsw_search_batch_refined(hnsw_index *h, hnsw_row_table *t, const float *Q /* nq x dim, or NULL */,
                              const float *Qfull /* nq x full_dim */, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef,
                              hnsw_mask_set *set /* or NULL */, const uint32_t *mask_of /* or NULL */,
                              const uint32_t *lo /* or NULL */, const uint32_t *hi /* or NULL */, uint32_t *ids /* nq x n */,
                              float *dists /* or NULL */, uint32_t *counts /* or NULL */, hnsw_query_stats *stats /* or NULL */);

/* ---- hybrid search: rank fusion of the index's hits with external ranked lists, on the device ---------------------------
 * An extension (the reference has one retriever): what Weaviate, Qdrant, Milvus and Elasticsearch call hybrid search.  The
 * dense index's hits are combined with ranked lists from other retrievers -- BM25, a sparse model, a second index over
 * another embedding -- by reciprocal rank fusion or by a weighted sum of scores.  The deletions, mask rows and label
 * ranges of this library live in its HBM and nowhere else, so the fusion applies them to EVERY list: an external
 * candidate this index holds as deleted, outside the query's label range or not visible under its mask row does not come
 * back, whichever retriever proposed it.  This is not hnsw_fuse_lists_device, which scores by distances to several
 * vectors and knows nothing of ranks, external scores or filters.
 * THE RANK FUSION of one query.
 * Lists.  A query has up to 8 ranked lists, in this order: the optional DENSE list, the index's own -- ids0 [nq][pool],
 * counts0 [nq] or NULL, stats0 [nq] or NULL; its distances are not an input -- then E EXTERNAL lists, 0 <= E <=
 * HNSW_HYBRID_MAX_EXT: ext_ids [nq][E][ext_width], ext_scores [nq][E][ext_width] f32 or NULL, ext_counts [nq][E] or NULL.
 * At least one list is given; total = (dense given ? pool : 0) + E * ext_width <= HNSW_FUSE_MAX_CANDS; 1 <= n_out <=
 * total.  weights [nq][1 + E] f32 or NULL: slot 0 is always the dense slot.  absent [E] f32 or NULL (every value 0.0f): a
 * HOST pointer in both entry points, read before the call returns.  Optionally the query's row Q [nq][dim], and
 * optionally a filter, the four arguments hnsw_search_batch_diverse takes: set, mask_of [nq], lo [nq], hi [nq].
 *   - entry j of a list is PRESENT as in THE FUSION: j < min(count, width), or, without counts, iff its id is not
 *     UINT32_MAX;
 *   - a FAILED query has count 0, unique 0, dropped 0 and padded rows.  The causes, in order of precedence: (1) the dense
 *     list's incoming status, if it is not HNSW_OK; (2) HNSW_ERR_ARG when mask_of[q] is neither HNSW_MASK_NONE nor below
 *     the set's n_masks (no mask word is read; mask_of NULL names row 0); (3) HNSW_ERR_ARG when any present id of any list
 *     is at or beyond the index length (no stored row, mask word or label is read for that query); (4)
 *     HNSW_ERR_NAN_INPUT when Q is given and Q[q] has a NaN element;
 *   - id i is ADMISSIBLE iff it is not deleted on the handle (ids beyond the deleted mask are not denied); and, with a
 *     set row, i < allow_bits and its bit is set (a HNSW_MASK_NONE query has no bit test); and, with a range, lo <=
 *     label(i) <= hi, where label(i) = 0 at or beyond the column's length (lo > hi admits nothing and reads no label):
 *     the predicate of the filtered searches;
 *   - the EFFECTIVE list: a list's present entries in order, the inadmissible ones removed, then every entry removed
 *     whose id an earlier kept entry of the same list already has.  rank(c) in a list is the 1-based position of c in
 *     what is left: what the caller would get had the other retriever applied the filter itself.  dropped = the present
 *     entries, over all lists, removed as inadmissible (repeats are not counted).  C = the distinct ids over all
 *     effective lists; unique = |C|;
 *   - mode HNSW_HYBRID_RRF: 1 <= rank_constant <= 2^20 (customarily 60; rank_constant + rank is then exact in f32).  For
 *     c in C, for each list that holds c, in list order (dense first): t = w / (float)(rank_constant + rank(c)), ONE
 *     correctly rounded f32 division, w the list's weight or 1.0f without weights; s is the first such term, then s = s +
 *     t, each add rounded on its own and never contracted; lists that do not hold c contribute nothing.  LARGER IS
 *     BETTER: ranked by (s descending under f32 >, -0 == +0; then id ascending).  Q does not enter the score;
 *   - mode HNSW_HYBRID_LINEAR: ext_scores is required when E > 0, and Q when E == 0; rank_constant is not read.  For c in
 *     C: x_dense = D(c), the bits of hnsw_distance_batch(h, Q[q], {c}) (the query-side arithmetic of the index's kind;
 *     under metric_cosine the unit copy, as THE FUSION does), evaluated for EVERY candidate whether or not the dense list
 *     holds it; x_e = the score of c's kept entry in external list e if that list holds c, else absent[e]; p = w * x one
 *     f32 multiply, omitted when weights is NULL.  With Q: s = p_dense, then s = s + p_e for e = 0 .. E-1.  With Q NULL
 *     the dense term is left out entirely and s starts at p_0: the dense list then only proposes candidates.  SMALLER IS
 *     BETTER: ranked by (s ascending under f32 <, -0 == +0; then id ascending); a caller gives similarity scores a
 *     negative weight;
 *   - both modes: a candidate whose score is NaN is never returned; infinite, zero and negative weights are legal; a NaN
 *     weight or a NaN external score is no argument error; the answer depends neither on which duplicate was kept nor on
 *     anything but (score, id).
 * Per query: ids [n_out] (pad UINT32_MAX), scores [n_out] (pad the mode's worst value: -inf under RRF, +inf under
 * LINEAR), dists [n_out] (optional, requires Q: D of each returned hit in either mode, pad +inf), counts, unique, dropped
 * (all optional), stats (required iff stats0 is given: the dense record with the status as above).  Every output word is
 * written exactly once.
 *
 * hnsw_fuse_ranked_device is THE RANK FUSION alone over buffers in HBM: every d_* pointer is device memory (`absent` is
 * host memory and travels by value), ids are local to the handle, so a replica handle serves.  After the snapshot -- and
 * whichever of the deleted mask, the label column and the set's words the call needs -- is brought up to date, ONE launch
 * (the distance seam's kernel in its rank-fusion form, one wave per query) is enqueued on `stream` and the call returns
 * without synchronising it.  Under the metric_cosine option it reads a stream-ordered unit-length copy of d_Q; otherwise
 * nothing is allocated or copied, and the call is capturable under hnsw_fuse_lists_device's conditions.  The status of a
 * failed query is written to d_stats only.  Outputs must not overlap inputs.  HNSW_ERR_ARG, decided before the device is
 * touched: h NULL; n_ext > HNSW_HYBRID_MAX_EXT; no list at all; total or n_out outside the limits; a mode other than the
 * two; RRF with rank_constant 0 or above 2^20; LINEAR without d_ext_scores when n_ext > 0, or without d_Q when n_ext ==
 * 0; d_ext_ids NULL with n_ext > 0; d_dists without d_Q; nq > 2^31 - 1; d_ids or d_scores NULL; exactly one of d_stats0 /
 * d_stats given; a set of another handle, d_mask_of without a set, one of d_lo / d_hi without the other; a set without
 * rows when d_mask_of is NULL.  nq == 0 is HNSW_OK on any handle, whatever else is passed, and launches nothing; an
 * empty index is HNSW_ERR_EMPTY.
 *
 * hnsw_search_batch_hybrid answers host-pointer queries.  By definition the result is THE RANK FUSION, with n_out = n,
 * Q given, of the dense list and the caller's external lists under the same filter, where the dense list is whatever the
 * right one of hnsw_search_batch / _filtered_set / _filtered_range / _filtered_set_range returns for Q with n = pool and
 * ef handed on exactly as hnsw_search_batch_diverse hands it on.  Everything of that call is inherited: deletions, the
 * cosine option, per-query errors (the first is returned with the query named; every other row is filled in).  With no
 * filter and nothing deleted the call stays on the device: Q and the external lists go up once, the launch of
 * hnsw_search_batch_device and the re-run loop of its _finish, one fusion launch, ONE copy of the block [ids | scores |
 * dists | counts | unique | dropped | stats] back.  Otherwise the candidates are the host form's and go up before the
 * fusion; pool <= 64 is then required.  scores, dists, counts, unique, dropped and stats may be NULL.  HNSW_ERR_ARG as the
 * primitive's, with 1 <= n <= pool + n_ext * ext_width, pool >= 1, Q and ids required.  hnsw_get_stat: "hybrid_calls"
 * (hnsw_search_batch_hybrid calls answered), "hybrid_fuse_launches" (rank fusions launched, hnsw_fuse_ranked_device's
 * included).
 * Not provided: min-max / z-score normalisation of scores; a different width per external list; label range lists;
 * fusion over shards; one-query gathered calls; the Rust shim's binding. */
#define HNSW_HYBRID_MAX_EXT 7
#define HNSW_HYBRID_RRF 0
#define HNSW_HYBRID_LINEAR 1
int hnsw_fuse_ranked_device(hnsw_index *h, uint64_t nq, uint32_t mode, uint32_t rank_constant, uint32_t n_out, uint32_t pool,
                            const uint32_t *d_ids0 /* nq x pool, or NULL */, const uint32_t *d_counts0 /* or NULL */,
                            const hnsw_query_stats *d_stats0 /* or NULL */, uint32_t n_ext, uint32_t ext_width,
                            const uint32_t *d_ext_ids /* nq x n_ext x ext_width */, const float *d_ext_scores /* or NULL */,
                            const uint32_t *d_ext_counts /* nq x n_ext, or NULL */,
                            const float *d_weights /* nq x (1 + n_ext), or NULL */, const float *absent /* host: n_ext, or NULL */,
                            const float *d_Q /* nq x dim, or NULL */, hnsw_mask_set *set /* or NULL */,
                            const uint32_t *d_mask_of /* or NULL */, const uint32_t *d_lo /* or NULL */,
                            const uint32_t *d_hi /* or NULL */, uint32_t *d_ids, float *d_scores /* nq x n_out */,
                            float *d_dists /* or NULL */, uint32_t *d_counts /* or NULL */, uint32_t *d_unique /* or NULL */,
                            uint32_t *d_dropped /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats0 */,
                            void *stream);
int hnsw_search_batch_hybrid(hnsw_index *h, const float *Q /* nq x dim */, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef,
                             uint32_t mode, uint32_t rank_constant, uint32_t n_ext, uint32_t ext_width,
                             const uint32_t *ext_ids /* nq x n_ext x ext_width */, const float *ext_scores /* or NULL */,
                             const uint32_t *ext_counts /* or NULL */, const float *weights /* nq x (1 + n_ext), or NULL */,
                             const float *absent /* n_ext, or NULL */, hnsw_mask_set *set /* or NULL */,
                             const uint32_t *mask_of /* or NULL */, const uint32_t *lo /* or NULL */,
                             const uint32_t *hi /* or NULL */, uint32_t *ids /* nq x n */, float *scores /* or NULL */,
                             float *dists /* or NULL */, uint32_t *counts /* or NULL */, uint32_t *unique /* or NULL */,
                             uint32_t *dropped /* or NULL */, hnsw_query_stats *stats /* or NULL */);

/* ---- boosted search: the pool re-ranked by per-id attributes kept in HBM ------------------------------------------------
 * An extension (the reference ranks by distance alone): what Elasticsearch calls function_score and Vespa a first-phase
 * rank profile.  "Near the query, but newer, more popular, in stock and not demoted" is a ranking by
 * w0 * distance + w1 * attr1[id] + w2 * attr2[id] + ...  The attributes belong to the id, so they live in HBM beside it:
 * a row table (refined search, above) with full_dim = A is an attribute table of A columns, written, read and grown by
 * the same calls.  This is not the rank fusion's linear mode, whose scores are per query and per list and go up with
 * every call.
 *
 * THE BOOST of one query, with a candidate list ids_in [pool] and dists_in [pool] (the distances ARE an input here),
 * counts_in or NULL, stats_in or NULL, a weight row w [1 + A] of f32 and a table of table_rows rows of A elements,
 * HNSW_ROWS_F32 or HNSW_ROWS_F16 (an f16 element is widened exactly where it is read):
 *   - entry j is PRESENT exactly as in THE REFINEMENT: iff j < min(count, pool), or, without counts, iff its id is not
 *     UINT32_MAX;
 *   - an incoming status that is not HNSW_OK fails the query with that status; otherwise a present id at or beyond
 *     table_rows gives HNSW_ERR_ARG, and no table row is read for the query.  A failed query has count 0 and padded rows;
 *   - the score of a present entry with distance d and row a is s = w[0] * d, then p = w[k + 1] * a[k]; s = s + p for
 *     k = 0 .. A - 1: ONE left-to-right f32 chain, every multiply and every add rounded on its own and never contracted
 *     into a fused multiply-add.  A result of -0.0f is taken as +0.0f and returned as +0.0f.  Infinite, zero and negative
 *     weights are legal, and a NaN weight is no argument error; an entry whose score is NaN is never returned, so a NaN
 *     weight returns nothing, and w[0] == 0 with d == +inf (0 * inf) DROPS the entry: pass a small positive w[0], not
 *     zero, to ignore finite distances while keeping unreachable candidates out of the way;
 *   - SMALLER IS BETTER: the present entries are ranked ascending by (s under f32 <, then id, then position in the
 *     incoming list); duplicate ids in a list are separate entries; -inf ranks first and +inf last, both returned.
 * Per query: ids [n_out] (pad UINT32_MAX), scores [n_out] (pad +inf), dists [n_out] (optional: the incoming distance of
 * each returned hit, pad +inf), counts (optional) = entries written, stats (required iff stats_in is given): the incoming
 * record unchanged but for the status above.  Every output word is written exactly once.  Limits: 1 <= n_out <= pool <=
 * HNSW_BOOST_POOL_MAX, 1 <= A <= HNSW_BOOST_MAX_ATTRS, nq <= 2^31 - 1; weights_rows is 1 (one row shared by every query)
 * or nq (weights [nq][1 + A]).
 *
 * hnsw_boost_device is THE BOOST alone over buffers in HBM.  It takes no handle, as hnsw_refine_device takes none: ONE
 * launch (the distance seam's kernel in its boost form, one wave per query) is enqueued on `stream` -- no synchronise, no
 * allocation, no copy.  d_table holds table_rows x n_attrs elements of dtype; outputs must not overlap inputs.  The status
 * of a failed query is written to d_stats only.  HNSW_ERR_ARG, decided before the device is touched: a limit violated; a
 * dtype other than the two; nq > 2^31 - 1; weights_rows not 1 or nq; d_table, d_weights, d_ids_in, d_dists_in, d_ids or
 * d_scores NULL; exactly one of d_stats_in / d_stats given.  nq == 0 is HNSW_OK whatever else is passed.
 *
 * hnsw_search_batch_boosted answers host-pointer queries.  By definition the result is THE BOOST, with n_out = n and A =
 * the table's full_dim, of the lists that the candidate call of hnsw_search_batch_diverse's table returns for Q with
 * n = pool and ef' = max(ef, pool, 1), and everything is inherited exactly as in hnsw_search_batch_refined: the filter
 * (set / mask_of / lo / hi), deleted ids taken out, the metric_cosine option, the planner, per-query errors, pool <= 64
 * and ef' <= 256 under a filter or deletions.  Unfiltered and with nothing deleted the call stays on the device: the
 * queries and the weights go up once, the launch of hnsw_search_batch_device and the re-run loop of its _finish, one boost
 * launch, ONE copy of the block [ids | scores | dists | counts | stats] back.  scores, dists, counts and stats may be
 * NULL.  HNSW_ERR_ARG, decided before the device is touched: the filter's own refusals; t NULL or of another handle; a
 * limit violated (a table of more than HNSW_BOOST_MAX_ATTRS columns is one); Q, weights or ids NULL; nq > 2^31 - 1;
 * weights_rows not 1 or nq; a table with fewer rows than the index; and, once the snapshot's device is known, a table on
 * another device.  nq == 0 is HNSW_OK; an empty index is HNSW_ERR_EMPTY.  hnsw_get_stat: "boost_calls"
 * (hnsw_search_batch_boosted calls answered), "boost_launches" (the boosts they launched, and hnsw_boost_device's: that
 * call has no handle, so its launches are counted for the process and every handle's key includes them).
 *
 * A row table in a file.  hnsw_save and hnsw_load do not carry a table; these two calls do, one file per table:
 *   hnsw_row_table_save   big-endian like the index's format: magic "HXRT" u32, version u32 = 1, full_dim u32, dtype u32,
 *                         rows u64, then rows x full_dim elements in the table's dtype.  The rows are read back from HBM
 *                         in chunks of at most 64 MiB.  A table that was never written saves rows = 0 and touches no
 *                         device.  HNSW_ERR_IO when the file cannot be created or written.
 *   hnsw_row_table_load   creates a table on h and writes the rows to it (the first chunk allocates, as a first write
 *                         does).  HNSW_ERR_IO for a file that cannot be opened, a bad magic or version, a full_dim or
 *                         dtype out of range, a file shorter or longer than its header says -- all decided before any
 *                         device is touched -- and for a NaN or infinite element; *out is then left alone.  The round
 *                         trip is bit-exact: -0, f16 subnormals and 65504 survive.
 * Not provided: more than 32 attributes; combiners other than the weighted sum (products, decay functions, clamps); a
 * boost over shards; one-query gathered calls; the Rust shim's binding; carrying a table through hnsw_clone or the
 * snapshot exchange (save it and load it on the other handle). */
#define HNSW_BOOST_POOL_MAX 1024
#define HNSW_BOOST_MAX_ATTRS 32
int hnsw_boost_device(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t n_attrs, uint32_t dtype,
                      const void *d_table /* table_rows x n_attrs of dtype */, uint64_t table_rows,
                      const float *d_weights /* weights_rows x (1 + n_attrs) */, uint64_t weights_rows /* 1 or nq */,
                      const uint32_t *d_ids_in /* nq x pool */, const float *d_dists_in /* nq x pool */,
                      const uint32_t *d_counts_in /* or NULL */, const hnsw_query_stats *d_stats_in /* or NULL */,
                      uint32_t *d_ids, float *d_scores /* nq x n_out */, float *d_dists /* or NULL */,
                      uint32_t *d_counts /* or NULL */, hnsw_query_stats *d_stats /* required iff d_stats_in */, void *stream);
int hnsw_search_batch_boosted(hnsw_index *h, hnsw_row_table *t, const float *Q /* nq x dim */, uint64_t nq, uint32_t n,
                              uint32_t pool, uint32_t ef, const float *weights /* weights_rows x (1 + full_dim) */,
                              uint64_t weights_rows /* 1 or nq */, hnsw_mask_set *set /* or NULL */,
                              const uint32_t *mask_of /* or NULL */, const uint32_t *lo /* or NULL */,
                              const uint32_t *hi /* or NULL */, uint32_t *ids /* nq x n */, float *scores /* or NULL */,
                              float *dists /* or NULL */, uint32_t *counts /* or NULL */, hnsw_query_stats *stats /* or NULL */);
int hnsw_row_table_save(hnsw_row_table *t, const char *path);
int hnsw_row_table_load(hnsw_index *h, const char *path, hnsw_row_table **out);

/* Test seams that mirror the reference's own units:
 * VecBase::dist2many (vectors/src/lib.rs:17-22): the query (quantised like ann_by_vector does,
 * template.rs:313) against stored ids, on the device, exact accumulation order. */
int hnsw_distance_batch(hnsw_index *h, const float *q, const uint32_t *ids, uint64_t k, float *out);
/* Searcher::search_layer (searcher.rs:23-103) on one layer from an explicit entry set. */
int hnsw_search_layer(hnsw_index *h, uint32_t layer, const float *q, const uint32_t *entry_ids,
                      uint32_t n_entry, uint32_t ef, uint32_t *out_ids, float *out_dists,
                      uint32_t *out_count, hnsw_query_stats *stats);
/* Exact top-k under the index's own metric by exhaustive scan on the device (the reference's
 * brute force: helpers/glove.rs:94-109, template.rs:531-541). */
int hnsw_brute_force(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids,
                     float *dists);
/* The same ground truth on the matrix cores, for sizes where the exact scan takes minutes (f32 rows,
 * dimension a multiple of 4, k <= 12): every point is screened by an MFMA score |x|^2 - 2 x.q
 * (v_mfma_f32_32x32x2_f32: f32 products and sums, but not FullVec::distance's summation order,
 * vectors/src/full.rs:23-29), the k + 8 best per query are re-evaluated in the reference's exact
 * arithmetic and sorted by (dist, id); equal scores are ordered by id, as equal distances are.  The
 * guarantee: with E = 1.01 (d + 2) 2^-24 max_x (|x|^2 + 2 sum|x_i||q_i|), the bound on the rounding error of
 * a score in any summation order, a query's result is hnsw_brute_force's, ids and distance bits, whenever for
 * each of its true k neighbours x at most k + 8 points (x included) have a true score within 2 E above
 * x's or below -- in particular whenever every score is exact in f32 (small integers).  Where the gaps are
 * smaller than that (rows far from the origin relative to their spread) the result is still k distinct
 * stored ids with the reference's own distances in (dist, id) order, but a neighbour can be missing.
 * tests/test_gpu_ground_truth.py holds both halves to the oracle, tests/ground_truth_inputs.py derives the
 * bound.  E models relative rounding and means nothing outside f32's normal range: a call in which a stored
 * row or a query has a largest |component| that is not zero and lies outside [2^-48, 2^40] is handed to
 * hnsw_brute_force whole (tests/test_gpu_numeric_range.py).  hnsw_brute_force is the unconditionally exact
 * scan.  An extension: the reference has no counterpart. */
int hnsw_brute_force_fast(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids,
                          float *dists);

/* ---- deletion (an extension: the reference has none; hnswlib's mark_deleted / unmark_deleted) -------------------
 * A deleted id stays a node of the graph: it is still traversed, still an entry point and still linked by later
 * builds (a tombstone), but NO SEARCH RETURNS IT.  hnsw_get_vector, hnsw_distance, the layer accessors,
 * hnsw_search_layer and hnsw_distance_batch (seams that mirror the reference's units) do not change.
 *   - Nothing deleted (hnsw_deleted_count == 0, also after every marked id was unmarked): every entry point takes
 *     exactly the code path, results and counters it takes without this feature.
 *   - Ids deleted: hnsw_search_batch (and hnsw_search, still coalesced: each caller gets what a lone
 *     hnsw_search_batch of its query returns) answers as hnsw_search_batch_filtered with every id < hnsw_len allowed
 *     and the deleted ids taken out -- ids, dists, counts and stats, path chosen by "filter_exact_max".  So n <= 64,
 *     ef' = max(ef, n, 1) <= 256 when the graph path is taken (else HNSW_ERR_ARG), and when ef < n the call returns
 *     up to n ids, not ef as without deletions.  Queries per path: hnsw_get_stat "deleted_queries_graph",
 *     "deleted_queries_exact", "deleted_overflow_exact".
 *     hnsw_search_batch_device always takes the graph path (enqueued on `stream`, no synchronisation) and _finish
 *     re-runs overflowing queries with larger tables, up to the graph path's largest, then answers those still
 *     overflowing by the exact path: the results of the host form with "filter_exact_max" = -1.
 *     hnsw_brute_force returns the top k of the undeleted ids (the filtered exact path: same arithmetic, same (dist,
 *     id) order, k <= 64); hnsw_brute_force_fast returns HNSW_ERR_ARG (its k + 8 re-rank cannot promise k live ids).
 *   - Marking and unmarking need no GPU: they change the host set and note the 64-id words they touched; the next
 *     search that needs the HBM copy sends only those words (no snapshot upload; "deleted_mask_words_uploaded").
 *     Like insert_*, they must not run concurrently with anything else on the handle.
 *   - hnsw_clone and hnsw_set_device carry the set; insert_*, import_points leave it as it is (new ids are live).
 *     hnsw_save writes it as the file `deleted` (see hnsw_save); hnsw_snapshot_describe / _adopt do not carry it:
 *     the set is per handle, a caller marks the same ids on every replica.
 * Not provided: reuse or compaction of deleted slots (hnswlib's replace_deleted), removal of nodes from the graph,
 * the Rust shim's binding. */
/* ids[k], each < hnsw_len (else HNSW_ERR_ARG and the set is unchanged); marking a deleted id again is a no-op */
int hnsw_mark_deleted(hnsw_index *h, const uint32_t *ids, uint64_t k);
int hnsw_unmark_deleted(hnsw_index *h, const uint32_t *ids, uint64_t k);
int hnsw_is_deleted(const hnsw_index *h, uint32_t id, int *out);
uint64_t hnsw_deleted_count(const hnsw_index *h);
/* the deleted ids, ascending, up to cap of them; *n receives the count (like hnsw_layer_nodes) */
int hnsw_get_deleted(const hnsw_index *h, uint32_t *ids, uint64_t cap, uint64_t *n);

/* ---- accessors ----------------------------------------------------------------------------- */
uint64_t hnsw_len(const hnsw_index *h);                                   /* template.rs:146 */
/* HNSW::distance(a, b) -> Option<f32>, template.rs:150-152: HNSW_ERR_ARG stands for None */
int hnsw_distance(const hnsw_index *h, uint32_t a, uint32_t b, float *out);
/* get_point(id).get_vals(): the (dequantised) values, template.rs:154, vectors/src/lib.rs:24-26 */
int hnsw_get_vector(const hnsw_index *h, uint32_t id, float *out);
int hnsw_get_level(const hnsw_index *h, uint32_t id, uint32_t *out);
/* raw QuantVec fields (vectors/src/quant.rs:6-11); HNSW_ERR_ARG for an F32 index */
int hnsw_get_quant(const hnsw_index *h, uint32_t id, uint8_t *codes, float *min_out, float *delta_out);
uint32_t hnsw_layer_count(const hnsw_index *h);                           /* layers.rs:21-23 */
uint64_t hnsw_layer_nb_nodes(const hnsw_index *h, uint32_t layer);        /* graph.rs:157-159 */
uint32_t hnsw_layer_m(const hnsw_index *h, uint32_t layer);               /* Graph.m, layers.rs:50 */
/* Graph::iter_nodes (graph.rs:27-29), ascending id; *n receives the node count */
int hnsw_layer_nodes(const hnsw_index *h, uint32_t layer, uint32_t *out, uint64_t cap, uint64_t *n);
/* Graph::neighbors / neighbors_vec / degree (graph.rs:96-113,150-155), ascending id */
int hnsw_neighbors(const hnsw_index *h, uint32_t layer, uint32_t id, uint32_t *buf, uint32_t cap,
                   uint32_t *deg);
/* whole layer as CSR over ascending node ids: node_ids[n_nodes], offsets[n_nodes + 1], nbrs[nnz];
 * pass NULL buffers to query the sizes. */
int hnsw_export_layer(const hnsw_index *h, uint32_t layer, uint32_t *node_ids, uint64_t *offsets,
                      uint32_t *nbrs, uint64_t *n_nodes, uint64_t *nnz);
/* HNSW::assert_param_compliance, template.rs:341-370: *ok = 1 when every degree <= ceil(1.1 *
 * limit) and no node of a multi-node layer is isolated */
int hnsw_check_param_compliance(const hnsw_index *h, int *ok);

/* ---- persistence ---------------------------------------------------------------------------- */
/* HNSW::save / HNSW::load, template.rs:43-131: directory with `points`, `params`, `layers/<n>`,
 * all big-endian, byte-compatible with the reference's Serializer impls (params.rs:78-114,
 * points.rs:124-145, point.rs:57-75, quant.rs:102-124, graph.rs:168-251).  With ids deleted, save also writes
 * the file `deleted` (count u64, then count ids u32 in strictly ascending order, big-endian), which the reference's
 * load ignores; with none it writes exactly the files above and removes a stale `deleted`.  load restores the set
 * and returns HNSW_ERR_IO for a `deleted` that is short, longer than its count, unsorted or holds an id >= len.
 * With some label nonzero (hnsw_set_labels), save also writes the file `labels` (count u64, then the labels of ids
 * 0..count-1 as u32, big-endian; trailing zero labels may be dropped); with every label zero it writes exactly the
 * files above and removes a stale `labels`.  load restores the column and returns HNSW_ERR_IO for a `labels` that is
 * short, longer than its count or has count > len. */
int hnsw_save(const hnsw_index *h, const char *dir);
int hnsw_load(const char *dir, hnsw_index **out);

/* ---- device management ---------------------------------------------------------------------- */
int hnsw_device_count(int *count);
/* bind the handle to a HIP device (default: the current device at first upload) */
int hnsw_set_device(hnsw_index *h, int device);
/* make the HBM snapshot current now (otherwise done lazily by the first search after a mutation) */
int hnsw_upload(hnsw_index *h);
int hnsw_device_bytes(const hnsw_index *h, uint64_t *bytes);
/* options of a handle; hnsw_clone copies every one of them to the clone.  The first two are tuning knobs of the HBM
 * snapshot (take effect at the next upload):
 *   "inline_rows"      -1 auto (default) / 0 never / 1 always: the layer-0 "inline rows" layout (a
 *                      copy of every neighbour's vector row next to the adjacency slot, so that one
 *                      expansion is one coalesced read; costs 2m x the row bytes of HBM)
 *   "inline_budget_mb" largest inline-rows allocation the auto mode accepts (default 65536)
 *   "gpu_build"        0 (default): hnsw_insert_bulk(_levels) is the CPU build; 2: it runs the on-device
 *                      build; 1: on-device searches with connect / prune on host threads (also what
 *                      hnsw_insert_bulk_device does while this is 1)
 *   "metric_cosine"    0 (default) / 1.  AN EXTENSION: the reference has Euclidean distance only
 *                      (vectors/src/lib.rs:10-27), so there is nothing to be bit-identical to -- parity unpinned.
 *                      With 1, every row is normalised to unit length as it is inserted and every query as it
 *                      arrives (one left-to-right f32 sum of squares, correctly rounded sqrt and division, the
 *                      same on host and device); behind that everything is the reference's L2 arithmetic, whose
 *                      order on unit vectors is the cosine order.  Distances returned are Euclidean distances
 *                      of the unit vectors (d^2 = 2 - 2 cos); hnsw_get_vector returns the stored unit rows; a
 *                      zero vector is HNSW_ERR_NAN_INPUT.  Set it before the first insert; save / load do not
 *                      carry it (the reference's file format has no such field): set it again after a load.
 *   "gpu_build_batch_max", "gpu_build_batch_div"
 *                      the on-device build inserts min(max, connected / div) points at a time (defaults
 *                      8192 and 8; max is capped at 32768); 256 and 64 stand closer to the reference's
 *                      one-at-a-time insertion (recall@10 + 0.0006 on the bench's index) for ~0.3 s more per
 *                      1M points; 32768 fills the machine better on indexes of tens of millions of points
 *                      (16M x 256d: 17.1 -> 15.4 s, recall unchanged) and when the insertion searches are
 *                      sharded over several GPUs
 *   "coalesce_us", "coalesce_depth", "coalesce_max"
 *                      the gathering of concurrent hnsw_search calls into one launch, see hnsw_search
 *   "filter_exact_max" hnsw_search_batch_filtered answers a call by the exact scan when its mask allows at most
 *                      this many ids (default 65536, from the crossover measured in DESIGN.md section 12; < 0: never)
 *   "filter_exact_grouped" 1: the batch filtered entry points run the exact-path groups of a call in three launches
 *                      for all of them instead of three per group (same results); 0, the default:
 *                      group by group; anything else is HNSW_ERR_ARG.  hnsw_search_filtered always groups
 *   "mask_set_cache_mb" HBM a resident mask set may hold in compacted id lists of its exact-path rows (per set,
 *                      default 64 -- a design choice, not a measurement; at the default "filter_exact_max" a list is
 *                      at most 256 KiB; 0: no list is kept) */
int hnsw_set_option(hnsw_index *h, const char *key, int64_t value);
/* counters of the handle: "uploads" (whole-snapshot uploads), "point_patches" (insert_vec calls that patched the
 * live snapshot), "patch_fallbacks" (those that could not: the next search uploads), "coalesced_batches" /
 * "coalesced_queries" / "coalesced_max_batch" (launches made for hnsw_search calls, the calls they answered, the
 * largest batch), "coalesce_ns_window" / "_turn" / "_gpu" / "_handout" (where the batch leaders' time went);
 * the on-device builds of the handle, summed: "build_points", "build_batches", "build_rows_read" (vector rows the
 * insertion searches and the heuristic read: distance evaluations + staged rows), "build_adj_rows" / "build_adj_ids"
 * (adjacency rows read and the ids in them), "build_records" / "build_removals" (edge records filed, reverse edges
 * dropped), "build_insert_kernel_us" (hx_insert_kernel, HIP events), "build_insert_phase_us" / "build_connect_us"
 * (host clock: phase 1 with its copies, sort + connect + remove), "build_connect_kernel_us" (hx_connect_kernel +
 * hx_remove_kernel, HIP events), and for the sharded build "build_rows_owned" /
 * "build_rows_received" (rows this rank changed as their owner and shipped; rows it received from the other owners),
 * "build_exchange_bytes" / "build_exchange_us" (the variable-size all-gathers: bytes received, host clock), and for the
 * device-connect build "build_cpu_path_points" (points its kernels could not serve: inserted on the CPU after it),
 * "build_rerun_points" (points whose insertion search filled the first, smaller visited table and ran again with a
 * larger one) and "build_kept_last_edges" (edges a prune dropped on one side only because they were the other
 * node's last edge -- the drop kernel's refusals plus the seed's clamp restores -- mirrored after the build; in the
 * sharded build every rank reports the whole build's, like "build_points"); hnsw_search_batch_filtered's (and
 * _multi's) queries by path: "filtered_queries_graph" (0), "filtered_queries_exact" (1), "filtered_overflow_exact" (2);
 * hnsw_search_batch_filtered_multi's calls and named masks: "filtered_multi_calls", "filtered_multi_masks"; resident
 * mask sets of the handle, summed: "mask_set_words_uploaded" (words of any set copied to HBM, by whole copies and by
 * scatters), "mask_set_recounts" (rows whose admissible ids the host counted), "mask_set_compactions" (compactions
 * launched for rows of a set), "filtered_set_calls" (hnsw_search_batch_filtered_set calls and completed
 * hnsw_search_batch_filtered_device calls); labels: "label_words_uploaded" (64-bit words of the label column copied
 * to HBM), "filtered_range_calls" (hnsw_search_batch_filtered_range calls and completed _range_device calls),
 * "filtered_range_ranges" (the distinct ranges they named), "filtered_set_range_calls"
 * (hnsw_search_batch_filtered_set_range calls and completed _set_range_device calls), "filtered_set_range_groups" (the
 * distinct (row, lo, hi) triples they named), "filtered_ranges_calls" (hnsw_search_batch_filtered_ranges calls and
 * completed _ranges_device calls), "filtered_ranges_groups" (the distinct canonical range lists they named),
 * "filtered_one_calls" / "filtered_one_batches" (hnsw_search_filtered calls answered, the launches of their leaders);
 * partitioned search, on the handle passed as shard 0: "shard_calls"
 * (hnsw_search_batch_shards calls whose shards were all searched), "shard_merges" (the merges they launched); grouped
 * search: "grouped_calls" (hnsw_search_batch_grouped calls answered), "grouped_launches" (collapses launched,
 * hnsw_group_by_label_device's included); radius search: "radius_calls" (hnsw_search_batch_radius calls answered),
 * "radius_rungs" (the search rungs they launched), "radius_launches" (the cuts they launched); diversified
 * search: "diverse_calls" (hnsw_search_batch_diverse calls answered), "diverse_launches" (selections launched,
 * hnsw_diversify_device's included); search from stored rows: "from_rows_calls" (hnsw_search_batch_from_rows and
 * _by_id calls answered), "from_rows_compose_launches" (hnsw_compose_rows_device's included), "from_rows_drop_launches"
 * (the drops those calls launched); multi-vector search: "multi_calls" (hnsw_search_batch_multi calls answered),
 * "multi_fuse_launches" (fusions launched, hnsw_fuse_lists_device's included); late-interaction search: "late_calls"
 * (hnsw_search_batch_late calls answered), "late_launches" (hnsw_late_interaction_device's included, and the composed
 * exact call's); exact document scoring: "docs_calls" (hnsw_search_batch_late_exact calls answered), "docs_launches"
 * (hnsw_score_documents_device's included), "doc_index_uploads" and "doc_index_keys_uploaded" (whole copies of the
 * document index to HBM, and the 8-byte keys they carried); hybrid search: "hybrid_calls" (hnsw_search_batch_hybrid
 * calls answered), "hybrid_fuse_launches" (rank fusions launched, hnsw_fuse_ranked_device's included); boosted search:
 * "boost_calls" (hnsw_search_batch_boosted calls answered), "boost_launches" (the boosts they launched, and every
 * hnsw_boost_device launch of the process: that call has no handle); deletion:
 * "deleted" (ids deleted now), "deleted_mask_words_uploaded" (64-id words of the deleted set copied to HBM), and the
 * unfiltered entry points' queries answered under deletions by path, "deleted_queries_graph" (0),
 * "deleted_queries_exact" (1), "deleted_overflow_exact" (2) */
int hnsw_get_stat(const hnsw_index *h, const char *key, uint64_t *out);

/* ---- replication of the HBM snapshot over the GPUs of a node ----------------------------------- */
/* The search path replicates the index per GPU (the reference keeps one index in
 * one process's RAM, template.rs:35-40).  The snapshot is a handful of flat device arrays plus a small
 * scalar header, so a replica is made by broadcasting them -- the caller's collective (ncclBroadcast over
 * xGMI; torch.distributed in hnsw_rs_amd/hnsw.py), the library only names the buffers:
 *   source rank:       hnsw_snapshot_describe(h, &d)   uploads if needed; d.bytes / d.ptr / d.header
 *   every other rank:  hnsw_create(same m, ef_cons, dim, kind), receive d.bytes and d.header,
 *                      hnsw_snapshot_adopt(h, &d)      allocates the arrays on the handle's device, fills d.ptr
 *                      <broadcast every array into d.ptr[i]>
 *                      hnsw_snapshot_commit(h)         the handle now answers searches
 * A handle made this way is a DEVICE-ONLY replica: it serves the search, brute-force and test-seam entry
 * points; it holds no host copy, so insert_*, save and the per-point / per-layer accessors fail with
 * HNSW_ERR_ARG (hnsw_len, hnsw_layer_count and hnsw_get_params answer from the header). */
#define HNSW_SNAPSHOT_ARRAYS 7
typedef struct hnsw_snapshot_desc {
    uint64_t bytes[HNSW_SNAPSHOT_ARRAYS]; /* size of each array, 0 = absent */
    void *ptr[HNSW_SNAPSHOT_ARRAYS];      /* device pointers on this handle's device */
    uint32_t header[32];                  /* scalar part, opaque: broadcast it verbatim */
} hnsw_snapshot_desc;
int hnsw_snapshot_describe(hnsw_index *h, hnsw_snapshot_desc *out);
int hnsw_snapshot_adopt(hnsw_index *h, hnsw_snapshot_desc *inout);
int hnsw_snapshot_commit(hnsw_index *h);

/* ---- kernel launch log: a test seam, off by default ------------------------------------------- */
/* Which kernel instantiations this process launched.  hnsw_kernel_log(1) clears the log and starts recording,
 * hnsw_kernel_log(0) stops.  While recording, every launch of every kernel (search, filtered, distance, brute
 * force, build) counts under the kernel it passed to the HIP runtime; the log is process-wide and thread-safe.
 * Off, a launch pays one relaxed atomic load.  hnsw_kernel_log_get writes one line per instantiation launched
 * since recording started, "<name> <count>\n", sorted by name; *needed = bytes including the terminating 0 (call
 * with buf = NULL, cap = 0 to size it; HNSW_ERR_ARG when cap is too small).  Names are hnsw_kernel_name's. */
int hnsw_kernel_log(int on);
int hnsw_kernel_log_get(char *buf, uint64_t cap, uint64_t *needed);
/* The name the log uses for a kernel symbol: demangled (when it is a mangled name), without the project's
 * namespaces, the return type and the parameter list, e.g. "hx_search_kernel<1, 64, 256, 4, false>". */
int hnsw_kernel_name(const char *name, char *buf, uint64_t cap, uint64_t *needed);

/* ---- harness helpers (not part of the reference's API) --------------------------------------- */
/* Synthetic "GloVe-shaped" data, counter-based so any row can be generated independently:
 * recipe 0 = low intrinsic dimension clusters (A), 1 = isotropic mixture (B), 2 = U[0,1)
 * (the reference's make_rand_vectors, template.rs:630-638).  out is n x d. */
int hnsw_synth_rows(int recipe, uint64_t seed, uint64_t first_row, uint64_t n, uint32_t d, float *out,
                    uint32_t nb_threads);
/* the level sampler used when levels are not given: believed-equivalent restatement of rand
 * 0.8.5 StdRng::seed_from_u64(0) -> gen::<f32>() -> floor(-ln(r) * ml) (points.rs:39-48,148-160) */
int hnsw_draw_levels(uint32_t m, uint64_t n, uint8_t *out);
/* The reference's call pattern as a load: `threads` host threads, each blocked in its own hnsw_search call
 * (ann_by_vector(&self, ...), template.rs:306-335, one query per call).  Thread t answers queries t, t + T, ... of
 * Q (nq x dim) again and again until `seconds` have passed and every query has been answered at least once.
 * ids (nq x n) / counts (nq, may be NULL) receive each query's last answer, *calls the number of completed calls,
 * *wall_s the elapsed time, lat_us[7] = {p50, p90, p99, max, mean} of the per-call latency in microseconds, then the
 * process's user and system CPU seconds over the run. */
int hnsw_bench_search_threads(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t threads,
                              double seconds, uint32_t *ids, uint32_t *counts, uint64_t *calls, double *wall_s,
                              double *lat_us);
/* The same around hnsw_search_filtered: query i is answered under row[i] of `set` (set and row both NULL: no set) and
 * the label range [lo[i], hi[i]].  dists (nq x n), counts, paths and rcs (nq each) may be NULL and receive each query's
 * last answer with ids; with rcs a per-query error (HNSW_ERR_NAN_INPUT) is that query's answer and the run goes on,
 * without it the first one ends the run.  Also the way to put real concurrency behind hnsw_search_filtered from a
 * language whose threads share an interpreter lock. */
int hnsw_bench_search_filtered_threads(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                       hnsw_mask_set *set, const uint32_t *row, const uint32_t *lo, const uint32_t *hi,
                                       uint32_t threads, double seconds, uint32_t *ids, float *dists, uint32_t *counts,
                                       uint8_t *paths, int32_t *rcs, uint64_t *calls, double *wall_s, double *lat_us);

/* `callers` host threads, each calling hnsw_search_batch(nq queries, host pointers) `calls` times on its own slice
 * of Q (total x dim) into its own result buffers; *wall_s = first call to last return (two untimed calls per caller
 * first).  What concurrent batch callers of the C ABI see. */
int hnsw_bench_batch_threads(hnsw_index *h, const float *Q, uint64_t total, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t callers, uint32_t calls, double *wall_s);

#ifdef __cplusplus
}
#endif
#endif
