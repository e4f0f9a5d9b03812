"""Boosted search (include/hnsw_mi355x.h, "boosted search"): a candidate list re-ranked by
w[0] * distance + w[1] * attr1[id] + w[2] * attr2[id] + ..., the attributes a row table of A columns -- float32, or
float16 widened exactly -- restated in numpy float32.  The library's own forms run on the device
(HNSW.search_batch_boosted, boost_device); boost_lists is what they are held to, bit for bit, and what a caller without a
GPU at hand can use on lists it already has."""
import numpy as np

from . import _lib
from ._lib import check
from .refine import dtype_of


def boost_lists(ids_in, dists_in, counts, statuses, table, weights, n_out):
    """THE BOOST of include/hnsw_mi355x.h.  ids_in [nq, pool] uint32, dists_in [nq, pool] float32, counts [nq] or None (an
    entry is then present iff its id is not UINT32_MAX), statuses [nq] or None (all OK), table [rows, A] float32 or float16
    (widened exactly), weights [1 + A] (one row for every query) or [nq, 1 + A] float32.  A query whose status is not OK
    keeps it; else a present id at or beyond the table's rows gives ERR_ARG (no row is read for that query).  Such a query
    has count 0 and padded rows.  Otherwise the score of a present entry is s = w[0] * d, then p = w[k + 1] * a[k];
    s = s + p over the attributes in order, every multiply and every add a float32 operation of its own; -0 becomes +0; the
    present entries are ranked ascending by (s, id, position), a NaN score is never returned, duplicate ids are separate
    entries, and the n_out smallest are returned.
    -> ids [nq, n_out] (pad UINT32_MAX), scores [nq, n_out] (pad +inf), dists [nq, n_out] (the incoming distances of the
    hits, pad +inf), counts [nq], statuses [nq]"""
    ids_in = np.ascontiguousarray(ids_in, dtype=np.uint32)
    dists_in = np.ascontiguousarray(dists_in, dtype=np.float32)
    table = np.asarray(table)
    if table.dtype not in (np.float32, np.float16):
        raise ValueError("the table is float32 or float16")
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    if ids_in.ndim != 2 or dists_in.shape != ids_in.shape or table.ndim != 2:
        raise ValueError("ids_in and dists_in are [nq, pool] and the table [rows, A]")
    nq, pool = ids_in.shape
    n_attrs, n_out = table.shape[1], int(n_out)
    if not 1 <= n_out <= pool <= _lib.BOOST_POOL_MAX or not 1 <= n_attrs <= _lib.BOOST_MAX_ATTRS:
        raise ValueError("1 <= n_out <= pool <= %d and 1 <= A <= %d" % (_lib.BOOST_POOL_MAX, _lib.BOOST_MAX_ATTRS))
    if weights.shape not in ((1 + n_attrs,), (1, 1 + n_attrs), (nq, 1 + n_attrs)):
        raise ValueError("weights are [1 + A] or [nq, 1 + A]")
    weights = weights.reshape(-1, 1 + n_attrs)
    if counts is not None:
        counts = np.asarray(counts).reshape(nq)
    st_in = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq)
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    o_status = st_in.copy()
    j = np.arange(pool)
    for q in range(nq):
        if st_in[q] != _lib.OK:
            continue
        present = ids_in[q] != _lib.UINT32_MAX if counts is None else j < min(int(counts[q]), pool)
        pos = np.flatnonzero(present)  # in list order, duplicates kept
        cand = ids_in[q][pos]
        if (cand.astype(np.int64) >= table.shape[0]).any():
            o_status[q] = _lib.ERR_ARG
            continue
        w = weights[q if weights.shape[0] > 1 else 0]
        if cand.size == 0:
            continue
        cols = np.ascontiguousarray(table[cand].astype(np.float32).T)  # [A, c]: an attribute of every candidate (exact)
        d = dists_in[q][pos]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            s = w[0] * d  # (the loop below is sequential over the attributes and vectorised over the candidates:
            for k in range(n_attrs):  # every element sees one float32 multiply and one float32 add per step)
                t = w[k + 1] * cols[k]
                s = s + t
        assert s.dtype == np.float32
        s[s == 0] = np.float32(0.0)  # -0 is +0
        live = np.flatnonzero(~np.isnan(s))
        b = s[live].view(np.uint32)
        key = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000))  # ascending as the float32 values are
        order = live[np.lexsort((pos[live], cand[live], key))][:n_out]
        k = order.size
        o_ids[q, :k], o_scores[q, :k], o_dists[q, :k], o_counts[q] = cand[order], s[order], d[order], k
    return o_ids, o_scores, o_dists, o_counts, o_status


def boost_device(nq, pool, n_out, n_attrs, dtype, d_table, table_rows, d_weights, weights_rows, d_ids_in, d_dists_in,
                 d_counts_in, d_stats_in, d_ids, d_scores, d_dists=None, d_counts=None, d_stats=None, stream=0):
    """hnsw_boost_device over torch device tensors (or raw device pointers): the [nq, pool] candidate ids and distances a
    *_device search left (d_counts_in / d_stats_in [nq] or None), re-ranked by the attributes of d_table -- table_rows x
    n_attrs elements of `dtype` ("f32" / "f16") -- under d_weights float32 [weights_rows, 1 + n_attrs] (weights_rows 1 or
    nq), into d_ids / d_scores [nq, n_out] (/ d_dists / d_counts / d_stats).  ONE launch enqueued on `stream` of the
    current device, no sync of it; needs no index."""
    from .hnsw import HNSW
    p = HNSW._dptr
    check(_lib.lib().hnsw_boost_device(
        nq, pool, n_out, n_attrs, dtype_of(dtype), p(d_table), table_rows, p(d_weights), weights_rows, p(d_ids_in),
        p(d_dists_in), p(d_counts_in), p(d_stats_in), p(d_ids), p(d_scores), p(d_dists), p(d_counts), p(d_stats),
        stream or None))
