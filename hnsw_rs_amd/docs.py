"""Exact document scoring (include/hnsw_mi355x.h, "exact document scoring"): the documents a list names -- a document is
the undeleted rows that share a label -- scored against a query of several vectors by summed min distance over EVERY
stored row of the document, restated in numpy float32.  The library's own forms run on the device
(HNSW.score_documents_device, HNSW.search_batch_late_exact); this is what they are held to, bit for bit, and what a caller
without a GPU at hand can use on labels it already has."""
import numpy as np

from . import _lib
from .late import mode_of


def score_documents(Q, mode, docs_in, counts, statuses, dist, labels, deleted, n_out, rows_cap, n_points):
    """THE DOCUMENT SCORING of include/hnsw_mi355x.h.  Q [nq, T, dim] float32, mode "sum" or "sum_sq", docs_in [nq, n_in]
    uint32 labels, counts [nq] or None (all n_in entries are then present: every uint32 is a label, there is no pad),
    statuses [nq] or None (all OK).  dist(q_row, ids) -> float32 [len(ids)]: the distances of one vector to stored ids in
    the index's own arithmetic, HNSW.distance_batch or OracleHNSW.distance_batch.  labels: the label column, uint32 [len]
    (an id at or beyond its length has label 0) or None (every label 0); deleted: the deleted ids, or None; n_points: the
    index length.
    A query with a status that is not OK keeps it; else a NaN element in any of its vectors gives ERR_NAN_INPUT.  Such a
    query has count 0, n_docs 0 and padded rows.  Otherwise the DISTINCT present labels that have an undeleted row below
    n_points are the documents; a document is scored over its min(doc_size, rows_cap) lowest ids: per vector the minimum
    over them (from +inf, a NaN distance leaving it as it is), e_t the minimum ("sum") or its square ("sum_sq"), s = e_0,
    then s = s + e_t in vector order; the n_out best documents by (score, -0 == +0; then label) are returned, a NaN score
    never.
    -> doc_labels [nq, n_out] (pad 0), scores [nq, n_out] (pad +inf), best_ids [nq, n_out] (pad UINT32_MAX: the scored row
    of the document with the smallest (distance bits, id) under any vector), doc_sizes [nq, n_out] (pad 0: the FULL size,
    whatever rows_cap), counts [nq], n_docs [nq], statuses [nq]"""
    mode = mode_of(mode)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    docs_in = np.ascontiguousarray(docs_in, dtype=np.uint32)
    if Q.ndim != 3 or docs_in.ndim != 2 or docs_in.shape[0] != Q.shape[0]:
        raise ValueError("Q is [nq, T, dim] and docs_in [nq, n_in]")
    nq, T = Q.shape[:2]
    n_in = docs_in.shape[1]
    n_out, rows_cap, n_points = int(n_out), int(rows_cap), int(n_points)
    if not 1 <= T <= _lib.LATE_MAX_VECS or not 1 <= n_out <= n_in <= _lib.DOCS_MAX_IN or not 1 <= rows_cap <= _lib.DOCS_MAX_ROWS:
        raise ValueError("1 <= T <= %d, 1 <= n_out <= n_in <= %d, 1 <= rows_cap <= %d"
                         % (_lib.LATE_MAX_VECS, _lib.DOCS_MAX_IN, _lib.DOCS_MAX_ROWS))
    if counts is not None:
        counts = np.asarray(counts).reshape(nq)
    st_in = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq)
    # the document index: the undeleted ids below n_points in (label, id) order
    lab_of = np.zeros(n_points, dtype=np.uint32)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)[:n_points]
        lab_of[:labels.size] = labels
    live = np.ones(n_points, dtype=bool)
    if deleted is not None:
        gone = np.asarray(deleted, dtype=np.int64).reshape(-1)
        live[gone[gone < n_points]] = False
    ids_live = np.flatnonzero(live).astype(np.uint32)
    ids_sorted = ids_live[np.argsort(lab_of[ids_live], kind="stable")]
    lab_sorted = lab_of[ids_sorted]
    o_labels = np.zeros((nq, n_out), dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_best = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_sizes = np.zeros((nq, n_out), dtype=np.uint32)
    o_counts, o_ndocs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        if st_in[q] != _lib.OK:
            o_status[q] = st_in[q]
            continue
        if np.isnan(Q[q]).any():
            o_status[q] = _lib.ERR_NAN_INPUT
            continue
        cnt = n_in if counts is None else min(int(counts[q]), n_in)
        named = np.unique(docs_in[q, :cnt])  # the distinct present labels, ascending
        first = np.searchsorted(lab_sorted, named, side="left")
        sizes = np.searchsorted(lab_sorted, named, side="right") - first
        has = sizes > 0
        docs, first, sizes = named[has], first[has], sizes[has]
        G = docs.size
        o_ndocs[q] = G
        if G == 0:
            continue
        scored = np.minimum(sizes, rows_cap)
        rows = np.concatenate([ids_sorted[a:a + k] for a, k in zip(first, scored)])  # a document's lowest ids
        of = np.repeat(np.arange(G), scored)
        s = None
        best = np.full(G, np.iinfo(np.uint64).max, dtype=np.uint64)  # (distance bits << 32 | id), the smallest
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(T):
                D = np.ascontiguousarray(dist(Q[q, t], rows), dtype=np.float32)
                m = np.full(G, np.inf, dtype=np.float32)
                ok = ~np.isnan(D)
                np.minimum.at(m, of[ok], D[ok])  # (no NaN among them: the minimum under f32 <)
                key = (D[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[ok].astype(np.uint64)
                np.minimum.at(best, of[ok], key)
                e = m * m if mode == _lib.LATE_SUM_SQ else m
                s = e if s is None else s + e
        s = s.astype(np.float32, copy=False)
        alive = np.flatnonzero(~np.isnan(s))
        order = alive[np.lexsort((docs[alive], np.where(s[alive] == 0, np.float32(0), s[alive])))][:n_out]
        k = order.size
        o_labels[q, :k], o_scores[q, :k], o_sizes[q, :k] = docs[order], s[order], sizes[order]
        o_best[q, :k] = (best[order] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        o_counts[q] = k
    return o_labels, o_scores, o_best, o_sizes, o_counts, o_ndocs, o_status
