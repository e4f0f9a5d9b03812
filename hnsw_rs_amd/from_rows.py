"""Search from stored rows (include/hnsw_mi355x.h, "search from stored rows"): the query rows composed out of stored
rows and the drop of the sources from the result lists, restated in numpy float32.  The library's own forms run on the
device (HNSW.search_batch_from_rows, HNSW.search_batch_by_id, HNSW.compose_rows_device, HNSW.drop_ids_device); this is
what they are held to, bit for bit, and what a caller without a GPU at hand can use on rows and lists it already has."""
import numpy as np

from . import _lib


def _slots(src_ids, weights):
    src_ids = np.ascontiguousarray(src_ids, dtype=np.uint32)
    if src_ids.ndim == 1:
        src_ids = src_ids.reshape(-1, 1)
    if src_ids.ndim != 2 or not 1 <= src_ids.shape[1] <= _lib.FROM_ROWS_MAX_TERMS:
        raise ValueError("src_ids is [nq, width], 1 <= width <= %d" % _lib.FROM_ROWS_MAX_TERMS)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(src_ids.shape[0], -1)
        if weights.shape != src_ids.shape:
            raise ValueError("weights has the shape of src_ids")
    return src_ids, weights


def compose_rows(src_ids, weights, get_row, n_points, dim=None):
    """THE COMPOSED QUERY of include/hnsw_mi355x.h for src_ids [nq, width] (a slot holding UINT32_MAX is absent) and
    weights [nq, width] float32 (None: every weight 1.0).  get_row(id) -> the stored row of an id as hnsw_get_vector
    returns it (HNSW.get_point(i).get_vals(), OracleHNSW.get_vals).  Element by element, over the present slots in slot
    order: acc = w * x for the first, acc = acc + (w * x) for every later one, each operation rounded to float32.  A query
    without a present slot, or with a present id at or beyond n_points, has the status ERR_ARG and a row of zeros, and no
    row is asked for.  dim: the rows' length, needed only when no query can be composed.
    -> rows [nq, dim] float32, statuses [nq] int32"""
    src_ids, weights = _slots(src_ids, weights)
    nq, width = src_ids.shape
    rows, statuses = None, np.zeros(nq, dtype=np.int32)
    todo = []
    for q in range(nq):
        present = [s for s in range(width) if src_ids[q, s] != _lib.UINT32_MAX]
        if not present or any(int(src_ids[q, s]) >= n_points for s in present):
            statuses[q] = _lib.ERR_ARG
            continue
        todo.append((q, present))
    cache = {}
    for q, present in todo:
        acc = None
        for s in present:
            i = int(src_ids[q, s])
            if i not in cache:
                cache[i] = np.ascontiguousarray(get_row(i), dtype=np.float32)
            w = np.float32(1.0) if weights is None else weights[q, s]
            with np.errstate(invalid="ignore", over="ignore"):
                p = w * cache[i]
                acc = p if acc is None else acc + p
        if rows is None:
            rows = np.zeros((nq, acc.shape[0]), dtype=np.float32)
        rows[q] = acc
    if rows is None:  # no query was composed
        if dim is None:
            raise ValueError("no query has a legal source: pass dim to get the rows of zeros")
        rows = np.zeros((nq, int(dim)), dtype=np.float32)
    return rows, statuses


def drop_ids(ids, dists, counts, statuses, ex, n_out, src_statuses=None):
    """THE DROP of include/hnsw_mi355x.h over ids / dists [nq, n_in] with the exclusion ids ex [nq, width] (UINT32_MAX:
    absent): entry j of a query is present iff j < min(counts[q], n_in), or, with counts None, iff its id is not
    UINT32_MAX; a query whose status (statuses [nq], or None: all OK) or compose status (src_statuses [nq], or None) is
    not OK has no present entry, and the compose status, when not OK, is the status it leaves with.  The present entries
    whose id equals no present exclusion id stay, in input order, cut to the first n_out.  Nothing is sorted.
    -> ids [nq, n_out] (pad UINT32_MAX), dists [nq, n_out] (the input's bits, pad +inf), counts [nq], dropped [nq]
    (present entries removed over all n_in), statuses [nq]"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    if ids.ndim != 2 or dists.shape != ids.shape:
        raise ValueError("ids and dists are [nq, n_in]")
    nq, n_in = ids.shape
    n_out = int(n_out)
    if not 1 <= n_out <= n_in <= _lib.DROP_MAX_N:
        raise ValueError("1 <= n_out <= n_in <= %d" % _lib.DROP_MAX_N)
    ex, _ = _slots(ex, None)
    if ex.shape[0] != nq:
        raise ValueError("ex is [nq, width]")
    statuses = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq)
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    dropped = np.zeros(nq, dtype=np.uint32)
    j = np.arange(n_in)
    for q in range(nq):
        ok = statuses[q] == _lib.OK
        if src_statuses is not None and int(np.asarray(src_statuses).reshape(nq)[q]) != _lib.OK:
            statuses[q] = int(np.asarray(src_statuses).reshape(nq)[q])
            ok = False
        if not ok:
            continue
        present = ids[q] != _lib.UINT32_MAX if counts is None else j < min(int(np.asarray(counts).reshape(nq)[q]), n_in)
        hit = np.isin(ids[q], ex[q][ex[q] != _lib.UINT32_MAX])
        dropped[q] = np.count_nonzero(present & hit)
        keep = np.flatnonzero(present & ~hit)[:n_out]
        o_ids[q, :keep.size], o_dists[q, :keep.size] = ids[q, keep], dists[q, keep]
        o_counts[q] = keep.size
    return o_ids, o_dists, o_counts, dropped, statuses
