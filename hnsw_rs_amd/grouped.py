"""Grouped search (include/hnsw_mi355x.h, "grouped search"): the collapse of candidate lists by label, restated in
numpy.  The library's own collapse runs on the device (HNSW.search_batch_grouped, HNSW.group_by_label_device); this is
what it is held to, entry for entry, and what a caller without a GPU at hand can use on lists it already has."""
import numpy as np

from . import _lib


def group_by_label(ids, dists, counts, labels, n_groups, per_group):
    """THE COLLAPSE of include/hnsw_mi355x.h over ids / dists [nq, pool]: entry j of a query is present iff
    j < min(counts[q], pool), or, with counts None, iff its id is not UINT32_MAX; its label is labels[id], 0 for an id
    at or beyond len(labels) (labels None: every label 0).  Nothing is sorted: ranks and group numbers follow position.
    -> ids [nq, n_groups, per_group] (pad UINT32_MAX), dists [nq, n_groups, per_group] (the input's bits, pad +inf),
    group_labels [nq, n_groups] (pad 0), group_sizes [nq, n_groups] (pad 0), counts [nq]"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    if ids.ndim != 2 or dists.shape != ids.shape:
        raise ValueError("ids and dists are [nq, pool]")
    nq, pool = ids.shape
    G, P = int(n_groups), int(per_group)
    if not (1 <= pool <= _lib.GROUP_POOL_MAX and 1 <= G <= pool and 1 <= P <= pool and G * P <= 1024):
        raise ValueError("1 <= n_groups, per_group <= pool <= %d and n_groups * per_group <= 1024" % _lib.GROUP_POOL_MAX)
    labels = np.zeros(0, dtype=np.uint32) if labels is None else np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    j = np.arange(pool)
    if counts is None:
        present = ids != _lib.UINT32_MAX
    else:
        present = j[None, :] < np.minimum(np.asarray(counts, dtype=np.int64).reshape(nq, 1), pool)
    inside = present & (ids < labels.shape[0])
    lab = np.zeros((nq, pool), dtype=np.uint32)
    lab[inside] = labels[ids[inside]]
    # same[q, j, i]: entries i and j of query q are both present and share a label
    same = (lab[:, :, None] == lab[:, None, :]) & present[:, :, None] & present[:, None, :]
    before = j[None, :] < j[:, None]  # [j, i]: i < j
    rank = (same & before[None]).sum(axis=2)
    first = np.where(present, same.argmax(axis=2), 0)  # the smallest i of the group (argmax: the first True)
    is_first = present & (rank == 0)
    n_first_before = np.concatenate([np.zeros((nq, 1), dtype=np.int64), np.cumsum(is_first, axis=1)[:, :-1]], axis=1)
    group = np.take_along_axis(n_first_before, first, axis=1)
    total = same.sum(axis=2)
    kept = present & (rank < P) & (group < G)
    o_ids = np.full((nq, G, P), _lib.UINT32_MAX, dtype=np.uint32)
    o_dists = np.full((nq, G, P), np.inf, dtype=np.float32)
    o_labels = np.zeros((nq, G), dtype=np.uint32)
    o_sizes = np.zeros((nq, G), dtype=np.uint32)
    qi, ji = np.nonzero(kept)
    o_ids[qi, group[qi, ji], rank[qi, ji]] = ids[qi, ji]
    o_dists[qi, group[qi, ji], rank[qi, ji]] = dists[qi, ji]
    qf, jf = np.nonzero(is_first & (group < G))
    o_labels[qf, group[qf, jf]] = lab[qf, jf]
    o_sizes[qf, group[qf, jf]] = np.minimum(total[qf, jf], P)
    o_counts = np.minimum(is_first.sum(axis=1), G).astype(np.uint32)
    return o_ids, o_dists, o_labels, o_sizes, o_counts
