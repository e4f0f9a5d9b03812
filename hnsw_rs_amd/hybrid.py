"""Hybrid search (include/hnsw_mi355x.h, "hybrid search"): the rank fusion of the index's own hits with ranked lists from
other retrievers, restated in numpy float32.  The library's own forms run on the device (HNSW.search_batch_hybrid,
HNSW.fuse_ranked_device); this is what they are held to, bit for bit, and what a caller without a GPU at hand can use on
lists it already has."""
import numpy as np

from . import _lib

MODES = {"rrf": _lib.HYBRID_RRF, "linear": _lib.HYBRID_LINEAR, _lib.HYBRID_RRF: _lib.HYBRID_RRF,
         _lib.HYBRID_LINEAR: _lib.HYBRID_LINEAR}
BAD_MASK = "bad mask"  # in place of a query's admissible callable: its mask_of names no row of the set (HNSW_ERR_ARG)


def mode_of(mode):
    """"rrf" / "linear" (or HYBRID_RRF / HYBRID_LINEAR) -> the ABI's mode word"""
    try:
        return MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode is 'rrf' or 'linear'")


def admissible_of(deleted=None, mask_row=None, labels=None, lo=None, hi=None):
    """The ADMISSIBLE predicate of one query -> admissible(ids) -> bool [len(ids)].  deleted: the ids deleted on the handle
    (or None); mask_row: bool [allow_bits], the query's row of its mask set (None: no bit test -- no set, or
    HNSW_MASK_NONE); labels: the label column, uint32 [<= len] (None: every label 0), with lo / hi the query's range
    (both None: no range).  An id at or beyond len(mask_row) is not admissible under a row; an id at or beyond len(labels)
    has label 0; lo > hi admits nothing."""
    dele = np.zeros(0, dtype=np.int64) if deleted is None else np.unique(np.asarray(deleted, dtype=np.int64))
    row = None if mask_row is None else np.asarray(mask_row, dtype=bool).reshape(-1)
    lab = np.zeros(0, dtype=np.uint32) if labels is None else np.asarray(labels, dtype=np.uint32).reshape(-1)
    if (lo is None) != (hi is None):
        raise ValueError("a label range needs lo and hi, both or neither")

    def admissible(ids):
        i = np.asarray(ids, dtype=np.int64).reshape(-1)
        ok = ~np.isin(i, dele)
        if row is not None:
            inside = i < row.shape[0]
            ok &= inside
            ok[inside] &= row[i[inside]]
        if lo is not None:
            l = np.zeros(i.shape[0], dtype=np.int64)
            known = i < lab.shape[0]
            l[known] = lab[i[known]]
            ok &= (l >= int(lo)) & (l <= int(hi))
        return ok
    return admissible


def filters_of(nq, deleted=None, masks=None, mask_of=None, labels=None, lo=None, hi=None):
    """One admissible callable per query (or BAD_MASK) out of a call's filter: masks bool [n_masks, allow_bits] (the rows of
    the mask set; None: no set), mask_of [nq] (rows, -1 or MASK_NONE; None: row 0), lo / hi [nq] or scalars (None: no
    range) -> list of nq entries for fuse_ranked"""
    out = []
    m = None if masks is None else np.asarray(masks, dtype=bool)
    if m is not None and m.ndim != 2:
        raise ValueError("masks is [n_masks, allow_bits]")
    for q in range(nq):
        row = None
        if m is not None:
            r = 0 if mask_of is None else int(np.asarray(mask_of).reshape(-1)[q])
            if r not in (-1, _lib.MASK_NONE):
                if not 0 <= r < m.shape[0]:
                    out.append(BAD_MASK)
                    continue
                row = m[r]
        a = None if lo is None else int(np.broadcast_to(np.asarray(lo), (nq,))[q])
        b = None if hi is None else int(np.broadcast_to(np.asarray(hi), (nq,))[q])
        out.append(admissible_of(deleted, row, labels, a, b))
    return out


def _order_kept(ids):
    """the first occurrence of every id, in list order"""
    _, first = np.unique(ids, return_index=True)
    return np.sort(first)


def fuse_ranked(mode, rank_constant, n_out, ids0, counts0, statuses0, ext_ids, ext_scores, ext_counts, weights, absent, Q,
                dist, admissible=None, n_points=None):
    """THE RANK FUSION of include/hnsw_mi355x.h.  mode "rrf" or "linear"; ids0 [nq, pool] uint32 or None (no dense list),
    counts0 [nq] or None (an entry is then present iff its id is not UINT32_MAX), statuses0 [nq] or None (all OK); ext_ids
    [nq, E, W] uint32 or None (E = 0), ext_scores [nq, E, W] float32 or None, ext_counts [nq, E] or None; weights
    [nq, 1 + E] float32 or None (slot 0 is the dense slot; RRF: numerator 1.0, LINEAR: no multiply); absent [E] float32 or
    None (zeros); Q [nq, dim] float32 or None.  dist(q_row, ids) -> float32 [len(ids)]: HNSW.distance_batch or
    OracleHNSW.distance_batch (asked only with Q: under LINEAR about every candidate, under RRF about the returned hits).
    admissible: None (every id), one callable ids -> bool[], or a sequence of nq of them with BAD_MASK where a query names
    no row of its set (admissible_of, filters_of).  n_points: the index length; None: no id is out of range.
    A failed query (the dense status; BAD_MASK; a present id at or beyond n_points; a NaN in Q[q] -- in this order) has
    count 0, unique 0, dropped 0 and padded rows.
    -> ids [nq, n_out] (pad UINT32_MAX), scores [nq, n_out] (pad -inf under rrf, +inf under linear), dists [nq, n_out] (pad
    +inf; None without Q), counts [nq], unique [nq], dropped [nq], statuses [nq]"""
    mode = mode_of(mode)
    f32 = np.float32
    lists = []  # (ids [nq, width], scores or None, counts or None) in list order, the dense one first
    if ids0 is not None:
        ids0 = np.ascontiguousarray(ids0, dtype=np.uint32)
        if ids0.ndim != 2:
            raise ValueError("ids0 is [nq, pool]")
    E = 0
    if ext_ids is not None:
        ext_ids = np.ascontiguousarray(ext_ids, dtype=np.uint32)
        if ext_ids.ndim != 3:
            raise ValueError("ext_ids is [nq, E, ext_width]")
        E = ext_ids.shape[1]
    if ids0 is None and E == 0:
        raise ValueError("at least one list: the dense one or an external one")
    nq = ids0.shape[0] if ids0 is not None else ext_ids.shape[0]
    total = (ids0.shape[1] if ids0 is not None else 0) + (E * ext_ids.shape[2] if E else 0)
    n_out = int(n_out)
    if E > _lib.HYBRID_MAX_EXT or not 1 <= total <= _lib.FUSE_MAX_CANDS or not 1 <= n_out <= total:
        raise ValueError("E <= %d, 1 <= n_out <= total <= %d" % (_lib.HYBRID_MAX_EXT, _lib.FUSE_MAX_CANDS))
    if mode == _lib.HYBRID_RRF and not 1 <= int(rank_constant) <= 1 << 20:
        raise ValueError("1 <= rank_constant <= 2^20")
    if mode == _lib.HYBRID_LINEAR and ((E and ext_scores is None) or (not E and Q is None)):
        raise ValueError("linear needs the external scores, or without an external list the queries")
    if ext_scores is not None:
        ext_scores = np.ascontiguousarray(ext_scores, dtype=np.float32).reshape(ext_ids.shape)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.shape != (nq, 1 + E):
            raise ValueError("weights is [nq, 1 + E]")
    ab = np.zeros(E, dtype=np.float32) if absent is None else np.ascontiguousarray(absent, dtype=np.float32).reshape(E)
    if Q is not None:
        Q = np.ascontiguousarray(Q, dtype=np.float32)
    st_in = np.zeros(nq, dtype=np.int64) if statuses0 is None else np.array(statuses0, dtype=np.int64).reshape(nq)
    worst = -np.inf if mode == _lib.HYBRID_RRF else np.inf
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_scores = np.full((nq, n_out), worst, dtype=np.float32)
    o_dists = None if Q is None else np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, o_unique, o_dropped = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
    o_status = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        if st_in[q] != _lib.OK:
            o_status[q] = st_in[q]
            continue
        adm = admissible[q] if isinstance(admissible, (list, tuple)) else admissible
        if isinstance(adm, str) and adm == BAD_MASK:
            o_status[q] = _lib.ERR_ARG
            continue
        present = []  # (slot of the weights, ids, scores or None) of every list, present entries in order
        if ids0 is not None:
            row = ids0[q]
            here = row != _lib.UINT32_MAX if counts0 is None else np.arange(row.shape[0]) < min(int(np.asarray(counts0).reshape(-1)[q]), row.shape[0])
            present.append((0, row[here], None))
        for e in range(E):
            row = ext_ids[q, e]
            here = row != _lib.UINT32_MAX if ext_counts is None else \
                np.arange(row.shape[0]) < min(int(np.asarray(ext_counts).reshape(nq, E)[q, e]), row.shape[0])
            present.append((1 + e, row[here], None if ext_scores is None else ext_scores[q, e][here]))
        if n_points is not None and any((i.astype(np.int64) >= int(n_points)).any() for _, i, _ in present):
            o_status[q] = _lib.ERR_ARG
            continue
        if Q is not None and np.isnan(Q[q]).any():
            o_status[q] = _lib.ERR_NAN_INPUT
            continue
        effective = []
        for slot, i, x in present:
            ok = np.ones(i.shape[0], dtype=bool) if adm is None else np.asarray(adm(i), dtype=bool)
            o_dropped[q] += int((~ok).sum())
            i, x = i[ok], (None if x is None else x[ok])
            keep = _order_kept(i)
            effective.append((slot, i[keep], None if x is None else x[keep]))
        cand = np.unique(np.concatenate([i for _, i, _ in effective]))  # ascending
        o_unique[q] = cand.size
        if cand.size == 0:
            continue
        with np.errstate(all="ignore"):
            if mode == _lib.HYBRID_RRF:
                s = np.zeros(cand.size, dtype=np.float32)
                have = np.zeros(cand.size, dtype=bool)
                for slot, i, _ in effective:
                    at = np.searchsorted(cand, i)
                    w = f32(1.0) if weights is None else weights[q, slot]
                    t = (w / (int(rank_constant) + 1 + np.arange(i.shape[0])).astype(np.float32)).astype(np.float32)
                    s[at] = np.where(have[at], s[at] + t, t)
                    have[at] = True
                key = -np.where(s == 0, f32(0), s)
            else:
                s = None
                if Q is not None:
                    D = np.ascontiguousarray(dist(Q[q], cand), dtype=np.float32)
                    s = D if weights is None else weights[q, 0] * D
                for slot, i, x in effective:
                    if slot == 0:
                        continue
                    xx = np.full(cand.size, ab[slot - 1], dtype=np.float32)
                    xx[np.searchsorted(cand, i)] = x
                    p = xx if weights is None else weights[q, slot] * xx
                    s = p if s is None else s + p
                s = s.astype(np.float32, copy=False)
                key = np.where(s == 0, f32(0), s)
        live = np.flatnonzero(~np.isnan(s))
        order = live[np.lexsort((cand[live], key[live]))][:n_out]
        o_ids[q, :order.size], o_scores[q, :order.size] = cand[order], s[order]
        o_counts[q] = order.size
        if Q is not None and order.size:
            o_dists[q, :order.size] = D[order] if mode == _lib.HYBRID_LINEAR else dist(Q[q], cand[order])
    return o_ids, o_scores, o_dists, o_counts, o_unique, o_dropped, o_status
