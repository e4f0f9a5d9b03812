"""Multi-vector search (include/hnsw_mi355x.h, "multi-vector search"): the fusion of a query's per-vector candidate
lists, restated in numpy float32.  The library's own forms run on the device (HNSW.search_batch_multi,
HNSW.fuse_lists_device); this is what they are held to, bit for bit, and what a caller without a GPU at hand can use on
lists it already has."""
import numpy as np

from . import _lib

MODES = {"sum": _lib.FUSE_SUM, "min": _lib.FUSE_MIN, _lib.FUSE_SUM: _lib.FUSE_SUM, _lib.FUSE_MIN: _lib.FUSE_MIN}


def mode_of(mode):
    """"sum" / "min" (or FUSE_SUM / FUSE_MIN) -> the ABI's mode word"""
    try:
        return MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode is 'sum' or 'min'")


def fuse_lists(Q, weights, mode, ids_in, counts, statuses, dist, n_out, n_points=None):
    """THE FUSION of include/hnsw_mi355x.h.  Q [nq, T, dim] float32, weights [nq, T] float32 or None (no multiply), mode
    "sum" or "min", ids_in [nq, T, pool] uint32, counts [nq, T] or None (an entry is then present iff its id is not
    UINT32_MAX), statuses [nq, T] or None (all OK).  dist(q_row, ids) -> float32 [len(ids)]: the distances of one vector to
    stored ids in the index's own arithmetic, HNSW.distance_batch or OracleHNSW.distance_batch (under the cosine option
    over what that callable expects: HNSW.distance_batch normalises the raw vector itself).  n_points: the index length;
    None: no id is out of range.
    A query with a status that is not OK keeps the first such status in vector order; else a present id at or beyond
    n_points gives ERR_ARG (dist is not asked about that query); else a NaN element in any of its vectors gives
    ERR_NAN_INPUT.  Such a query has count 0, unique 0 and padded rows.  Otherwise every DISTINCT present id is scored
    against every vector, p = w * D as one float32 multiply, folded in vector order -- sum: s = p_0, then s = s + p_t; min:
    s = +inf, then s = p_t if p_t < s -- and the n_out best by (score, -0 == +0; then id) are returned; a NaN score never is.
    -> ids [nq, n_out] (pad UINT32_MAX), scores [nq, n_out] (pad +inf), counts [nq], unique [nq], statuses [nq]"""
    mode = mode_of(mode)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    ids_in = np.ascontiguousarray(ids_in, dtype=np.uint32)
    if Q.ndim != 3 or ids_in.ndim != 3 or ids_in.shape[:2] != Q.shape[:2]:
        raise ValueError("Q is [nq, T, dim] and ids_in [nq, T, pool]")
    nq, T, pool = ids_in.shape
    n_out = int(n_out)
    if not 1 <= T <= _lib.MULTI_MAX_VECS or not 1 <= n_out <= pool or T * pool > _lib.FUSE_MAX_CANDS:
        raise ValueError("1 <= T <= %d, 1 <= n_out <= pool, T * pool <= %d" % (_lib.MULTI_MAX_VECS, _lib.FUSE_MAX_CANDS))
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.shape != (nq, T):
            raise ValueError("weights is [nq, T]")
    if counts is not None:
        counts = np.asarray(counts).reshape(nq, T)
    st_in = np.zeros((nq, T), dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq, T)
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, o_unique = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
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
        o_unique[q] = cand.size
        if cand.size == 0:
            continue
        s = None
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(T):
                p = np.ascontiguousarray(dist(Q[q, t], cand), dtype=np.float32)
                if weights is not None:
                    p = weights[q, t] * p
                if mode == _lib.FUSE_SUM:
                    s = p if s is None else s + p
                else:
                    s = np.full(cand.size, np.inf, dtype=np.float32) if s is None else s
                    s = np.where(p < s, p, s)
        s = s.astype(np.float32, copy=False)
        live = np.flatnonzero(~np.isnan(s))
        order = live[np.lexsort((cand[live], np.where(s[live] == 0, np.float32(0), s[live])))][:n_out]
        o_ids[q, :order.size], o_scores[q, :order.size] = cand[order], s[order]
        o_counts[q] = order.size
    return o_ids, o_scores, o_counts, o_unique, o_status
