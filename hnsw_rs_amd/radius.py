"""Radius search (include/hnsw_mi355x.h, "radius search"): the cut of candidate lists at a radius and the doubling
ladder over it, restated in numpy.  The library's own cut runs on the device (HNSW.search_batch_radius,
HNSW.radius_cut_device); this is what it is held to, entry for entry, and what a caller without a GPU at hand can use on
lists it already has -- the ladder runs over any search callable, the CPU oracle's included."""
import numpy as np

from . import _lib


def _stats4(stats, nq):
    """a stats array [nq, 3] (no status column: every query HNSW_OK) or [nq, 4] -> int64 [nq, 4]; None stays None"""
    if stats is None:
        return None
    stats = np.asarray(stats)
    if stats.ndim != 2 or stats.shape[0] != nq or stats.shape[1] not in (3, 4):
        raise ValueError("stats are [nq, 3] or [nq, 4]")
    out = np.zeros((nq, 4), dtype=np.int64)
    out[:, :stats.shape[1]] = stats.astype(np.int64)
    return out


def radius_cut(ids, dists, counts, stats, radius, n_out):
    """THE CUT of include/hnsw_mi355x.h over ids / dists [nq, n_in]: entry j of a query is present iff
    j < min(counts[q], n_in), or, with counts None, iff its id is not UINT32_MAX; a present entry is kept iff
    dist <= radius[q] as f32 (a NaN on either side keeps nothing).  Nothing is sorted: the kept entries stay in their
    input order.  stats [nq, 4] (or [nq, 3]: no status column) or None: a query whose status is not 0 has nothing present.
    radius: [nq] or a scalar.
    -> ids [nq, n_out] (pad UINT32_MAX), dists [nq, n_out] (the input's bits, pad +inf), counts [nq], flags [nq]
    (RADIUS_MORE iff the status is 0, all n_in entries are present and all were kept), stats (int64 [nq, 4], or None)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    if ids.ndim != 2 or dists.shape != ids.shape:
        raise ValueError("ids and dists are [nq, n_in]")
    nq, n_in = ids.shape
    n_out = int(n_out)
    if not 1 <= n_in <= n_out <= _lib.RADIUS_MAX_N:
        raise ValueError("1 <= n_in <= n_out <= %d" % _lib.RADIUS_MAX_N)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    stats = _stats4(stats, nq)
    ok = np.ones(nq, dtype=bool) if stats is None else stats[:, 3] == 0
    j = np.arange(n_in)
    if counts is None:
        present = ids != _lib.UINT32_MAX
    else:
        present = j[None, :] < np.minimum(np.asarray(counts, dtype=np.int64).reshape(nq, 1), n_in)
    present = present & ok[:, None]
    with np.errstate(invalid="ignore"):
        kept = present & (dists <= radius[:, None])
    w = kept.sum(axis=1)
    order = np.argsort(~kept, axis=1, kind="stable")  # the kept entries first, in their input order
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_bits = np.full((nq, n_out), 0x7F800000, dtype=np.uint32)
    have = j[None, :] < w[:, None]
    o_ids[:, :n_in][have] = np.take_along_axis(ids, order, axis=1)[have]
    o_bits[:, :n_in][have] = np.take_along_axis(dists.view(np.uint32), order, axis=1)[have]
    flags = np.where(ok & (present.sum(axis=1) == n_in) & (w == n_in), _lib.RADIUS_MORE, 0).astype(np.uint32)
    return o_ids, o_bits.view(np.float32), w.astype(np.uint32), flags, stats


def radius_ladder(search, Q, radius, n_first, max_n, ef):
    """THE LADDER of include/hnsw_mi355x.h over any search(Q_sub, n, ef) -> (ids [nq, n], dists, counts, stats [nq, 3 or
    4], ...): rung k searches the unfinished queries with n_k = min(n_first << k, max_n) and ef_k = max(ef, n_k) and cuts
    their lists at their radii; a query stops when its status is not 0, its cut does not set RADIUS_MORE, or n_k == max_n.
    -> ids [nq, max_n], dists [nq, max_n], counts [nq], flags [nq] (RADIUS_MORE: truncated at max_n), rungs [nq],
    stats int64 [nq, 4] (the last rung's)"""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, n_first, max_n, ef = Q.shape[0], int(n_first), int(max_n), int(ef)
    if not 1 <= n_first <= max_n <= _lib.RADIUS_MAX_N:
        raise ValueError("1 <= n_first <= max_n <= %d" % _lib.RADIUS_MAX_N)
    radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
    if not (radius >= 0).all():
        raise ValueError("every radius is >= 0 and not NaN")
    ids = np.full((nq, max_n), _lib.UINT32_MAX, dtype=np.uint32)
    dists = np.full((nq, max_n), np.inf, dtype=np.float32)
    counts, flags, rungs = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
    stats = np.zeros((nq, 4), dtype=np.int64)
    sel = np.arange(nq)
    k = 0
    while sel.size:
        n_k = min(n_first << k, max_n)
        got = search(Q[sel], n_k, max(ef, n_k))
        st = _stats4(got[3], sel.size)
        ids[sel], dists[sel], counts[sel], flags[sel], stats[sel] = radius_cut(got[0], got[1], got[2], st, radius[sel], max_n)
        rungs[sel] = k + 1
        if n_k == max_n:
            break
        sel = sel[(flags[sel] & _lib.RADIUS_MORE) != 0]
        k += 1
    return ids, dists, counts, flags, rungs, stats


def to_csr(ids, dists, counts):
    """the padded rows of a radius search -> (lims uint64 [nq + 1], ids, dists), FAISS's range_search layout: the answer
    of query q is ids[lims[q]:lims[q + 1]] / dists[lims[q]:lims[q + 1]]"""
    ids, dists = np.asarray(ids), np.asarray(dists)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if ids.ndim != 2 or dists.shape != ids.shape or counts.shape[0] != ids.shape[0] or (counts > ids.shape[1]).any():
        raise ValueError("ids and dists are [nq, n], counts [nq] with every count <= n")
    lims = np.zeros(ids.shape[0] + 1, dtype=np.uint64)
    lims[1:] = np.cumsum(counts)
    have = np.arange(ids.shape[1])[None, :] < counts[:, None]
    return lims, ids[have], dists[have]
