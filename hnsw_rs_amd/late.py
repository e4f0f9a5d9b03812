"""Late-interaction search (include/hnsw_mi355x.h, "late-interaction search"): a query's per-vector candidate lists scored
as documents -- the candidates that share a label -- by summed min distance, restated in numpy float32.  The library's
own forms run on the device (HNSW.search_batch_late, HNSW.late_interaction_device); this is what they are held to, bit
for bit, and what a caller without a GPU at hand can use on lists it already has."""
import numpy as np

from . import _lib

MODES = {"sum": _lib.LATE_SUM, "sum_sq": _lib.LATE_SUM_SQ, _lib.LATE_SUM: _lib.LATE_SUM, _lib.LATE_SUM_SQ: _lib.LATE_SUM_SQ}


def mode_of(mode):
    """"sum" / "sum_sq" (or LATE_SUM / LATE_SUM_SQ) -> the ABI's mode word"""
    try:
        return MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode is 'sum' or 'sum_sq'")


def late_interaction(Q, mode, ids_in, counts, statuses, dist, labels, n_out, n_points=None):
    """THE LATE INTERACTION of include/hnsw_mi355x.h.  Q [nq, T, dim] float32, mode "sum" or "sum_sq", ids_in [nq, T, pool]
    uint32, counts [nq, T] or None (an entry is then present iff its id is not UINT32_MAX), statuses [nq, T] or None (all
    OK).  dist(q_row, ids) -> float32 [len(ids)]: the distances of one vector to stored ids in the index's own arithmetic,
    HNSW.distance_batch or OracleHNSW.distance_batch.  labels: the label column, uint32 [len] (an id at or beyond its
    length has label 0) or None (every label 0: one document).  n_points: the index length; None: no id is out of range.
    A query with a status that is not OK keeps the first such status in vector order; else a present id at or beyond
    n_points gives ERR_ARG (dist is not asked about that query); else a NaN element in any of its vectors gives
    ERR_NAN_INPUT.  Such a query has count 0, n_docs 0 and padded rows.  Otherwise the DISTINCT present ids are the
    candidates, the distinct labels among them the documents; per vector a document's minimum over its candidates
    (from +inf, a NaN distance leaving it as it is), e_t the minimum ("sum") or its square ("sum_sq"), s = e_0, then
    s = s + e_t in vector order; the n_out best documents by (score, -0 == +0; then label) are returned, a NaN score never.
    -> doc_labels [nq, n_out] (pad 0), scores [nq, n_out] (pad +inf), best_ids [nq, n_out] (pad UINT32_MAX: the candidate
    of the document with the smallest (distance bits, id) under any vector), doc_sizes [nq, n_out] (pad 0), counts [nq],
    n_docs [nq], statuses [nq]"""
    mode = mode_of(mode)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    ids_in = np.ascontiguousarray(ids_in, dtype=np.uint32)
    if Q.ndim != 3 or ids_in.ndim != 3 or ids_in.shape[:2] != Q.shape[:2]:
        raise ValueError("Q is [nq, T, dim] and ids_in [nq, T, pool]")
    nq, T, pool = ids_in.shape
    n_out = int(n_out)
    if not 1 <= T <= _lib.LATE_MAX_VECS or T * pool > _lib.LATE_MAX_CANDS or not 1 <= n_out <= min(T * pool, _lib.LATE_MAX_DOCS):
        raise ValueError("1 <= T <= %d, T * pool <= %d, 1 <= n_out <= min(T * pool, %d)"
                         % (_lib.LATE_MAX_VECS, _lib.LATE_MAX_CANDS, _lib.LATE_MAX_DOCS))
    if counts is not None:
        counts = np.asarray(counts).reshape(nq, T)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    st_in = np.zeros((nq, T), dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq, T)
    o_labels = np.zeros((nq, n_out), dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_best = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_sizes = np.zeros((nq, n_out), dtype=np.uint32)
    o_counts, o_ndocs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64)
    j = np.arange(pool)
    for q in range(nq):
        bad = np.flatnonzero(st_in[q] != _lib.OK)
        if bad.size:
            o_status[q] = st_in[q, bad[0]]
            continue
        if counts is None:
            present = ids_in[q] != _lib.UINT32_MAX
        else:
            present = j[None, :] < np.minimum(counts[q].astype(np.int64), pool)[:, None]
        cand = np.unique(ids_in[q][present])  # the distinct present ids, ascending
        if n_points is not None and (cand.astype(np.int64) >= int(n_points)).any():
            o_status[q] = _lib.ERR_ARG
            continue
        if np.isnan(Q[q]).any():
            o_status[q] = _lib.ERR_NAN_INPUT
            continue
        if cand.size == 0:
            continue
        lab = np.zeros(cand.size, dtype=np.uint32)
        if labels is not None:
            inside = cand < labels.size
            lab[inside] = labels[cand[inside]]
        docs, of, sizes = np.unique(lab, return_inverse=True, return_counts=True)  # the documents, by label ascending
        of = of.reshape(-1)
        G = docs.size
        o_ndocs[q] = G
        s = None
        best = np.full(G, np.iinfo(np.uint64).max, dtype=np.uint64)  # (distance bits << 32 | id), the smallest
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(T):
                D = np.ascontiguousarray(dist(Q[q, t], cand), dtype=np.float32)
                m = np.full(G, np.inf, dtype=np.float32)
                ok = ~np.isnan(D)
                np.minimum.at(m, of[ok], D[ok])  # (no NaN among them: the minimum under f32 <)
                key = (D[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand[ok].astype(np.uint64)
                np.minimum.at(best, of[ok], key)
                e = m * m if mode == _lib.LATE_SUM_SQ else m
                s = e if s is None else s + e
        s = s.astype(np.float32, copy=False)
        live = np.flatnonzero(~np.isnan(s))
        order = live[np.lexsort((docs[live], np.where(s[live] == 0, np.float32(0), s[live])))][:n_out]
        k = order.size
        o_labels[q, :k], o_scores[q, :k], o_sizes[q, :k] = docs[order], s[order], sizes[order]
        o_best[q, :k] = (best[order] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        o_counts[q] = k
    return o_labels, o_scores, o_best, o_sizes, o_counts, o_ndocs, o_status
