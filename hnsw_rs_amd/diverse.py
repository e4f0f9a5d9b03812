"""Diversified search (include/hnsw_mi355x.h, "diversified search"): the re-ranking of candidate lists by maximal
marginal relevance, restated in numpy float32.  The library's own selection runs on the device
(HNSW.search_batch_diverse, HNSW.diversify_device); this is what it is held to, bit for bit, and what a caller without a
GPU at hand can use on lists it already has."""
import numpy as np

from . import _lib


def mmr_select(ids, dists, counts, statuses, pair_dist, lam, n_out, n_points=None):
    """THE SELECTION of include/hnsw_mi355x.h over ids / dists [nq, pool]: entry j of a query is present iff
    j < min(counts[q], pool), or, with counts None, iff its id is not UINT32_MAX; a query whose status (statuses [nq],
    or None: all OK) is not OK has no present entry.  pair_dist(a, b) -> the distance between stored rows a and b, the
    selected row first (HNSW.distance, OracleHNSW.distance); it is asked once per (selected, candidate) pair, in
    float32.  n_points: when given, a present id at or beyond it gives its query the status ERR_ARG and nothing else.
    Step t takes the present, unselected entry with the smallest
        score = (lam * dist) - ((1 - lam) * m),   m = 0 at t = 0, else the minimum of pair_dist(selected, entry) so far,
    every operation rounded to float32, ties to the lower position, a NaN score never.  Nothing is sorted.
    -> ids [nq, n_out] (pad UINT32_MAX), dists [nq, n_out] (the input's bits, pad +inf), gaps [nq, n_out] (m of the entry
    when it was selected; +inf for the first and the pad), counts [nq], statuses [nq], in selection order"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    if ids.ndim != 2 or dists.shape != ids.shape:
        raise ValueError("ids and dists are [nq, pool]")
    nq, pool = ids.shape
    n_out = int(n_out)
    if not 1 <= n_out <= pool <= _lib.DIVERSE_POOL_MAX:
        raise ValueError("1 <= n_out <= pool <= %d" % _lib.DIVERSE_POOL_MAX)
    lam = np.float32(lam)
    if not (lam >= 0 and lam <= 1):
        raise ValueError("lambda lies in [0, 1]")
    rest = np.float32(1.0) - lam
    statuses = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq)
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_gaps = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    j = np.arange(pool)
    for q in range(nq):
        if statuses[q] != _lib.OK:
            continue
        alive = ids[q] != _lib.UINT32_MAX if counts is None else j < min(int(np.asarray(counts).reshape(nq)[q]), pool)
        if n_points is not None and (ids[q][alive] >= n_points).any():
            statuses[q] = _lib.ERR_ARG
            continue
        alive = alive.copy()
        running = np.full(pool, np.inf, dtype=np.float32)
        for t in range(n_out):
            if t > 0:
                s = int(o_ids[q, t - 1])
                idx = np.flatnonzero(alive)
                D = np.array([pair_dist(s, int(ids[q, i])) for i in idx], dtype=np.float32)
                running[idx] = np.where(D < running[idx], D, running[idx])
            m = np.zeros(pool, dtype=np.float32) if t == 0 else running
            with np.errstate(invalid="ignore", over="ignore"):
                score = (lam * dists[q]) - (rest * m)
            idx = np.flatnonzero(alive & ~np.isnan(score))
            if idx.size == 0:
                break
            best = idx[np.argmin(score[idx])]  # (the first of the smallest under <: -0 == +0, ties to the lower position)
            o_ids[q, t], o_dists[q, t], o_gaps[q, t] = ids[q, best], dists[q, best], running[best]
            alive[best] = False
            o_counts[q] = t + 1
    return o_ids, o_dists, o_gaps, o_counts, statuses
