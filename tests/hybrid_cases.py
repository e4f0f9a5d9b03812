"""What the hybrid search tests share (tests/test_hybrid_host.py, tests/test_gpu_hybrid.py): a plain-loop restatement of
THE RANK FUSION of include/hnsw_mi355x.h, written independently of hnsw_rs_amd.hybrid.fuse_ranked (scalar float32
arithmetic, one candidate at a time, no numpy sorting, its own admissibility test), the synthetic ranked lists of the
sweep with their planted queries, the synthetic filter and the weight kinds.  A helper of the tests, no tests of its
own."""
import numpy as np

from tests import multi_cases as MC

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG, ERR_OVERFLOW = 0, -2, -8, -11
RRF, LINEAR = 0, 1
NQ = 16         # queries per synthetic call; the first N_PLANTED are the planted ones
N_PLANTED = 12
ID_SPAN = MC.ID_SPAN  # the synthetic lists draw their ids below this (the "index length" of the host sweep)
ALLOW_BITS = 280      # ids a mask row covers: below the length, so that lists hold ids at and beyond it
LABEL_LEN = 290       # the label column's length: below the length too
N_MASKS = 3
# (dense pool or 0, external lists, their width): no dense list, E = 0, E = 7, pool != width, the table's end
SHAPES = [(1, 0, 0), (0, 1, 1), (16, 1, 16), (10, 2, 7), (0, 3, 20), (4, 7, 36), (64, 3, 64), (200, 0, 0), (0, 7, 5), (31, 1, 2)]
FILTER_KINDS = ("none", "deleted", "set", "range", "both")
WEIGHT_KINDS = ("none", "ones", "mixed")


def n_outs(total):
    return sorted({1, min(10, total), total})


def table_dist():
    """multi_cases' synthetic distance: a query names a row of a table in its element 0"""
    return MC.table_dist()


def _admissible(i, deleted, row, labels, lo, hi):
    if i in deleted:
        return False
    if row is not None and (i >= len(row) or not row[i]):
        return False
    if lo is not None:
        if lo > hi:
            return False
        lab = int(labels[i]) if labels is not None and i < len(labels) else 0
        if not lo <= lab <= hi:
            return False
    return True


def naive(mode, rank_constant, n_out, ids0, counts0, statuses0, ext_ids, ext_scores, ext_counts, weights, absent, Q, dist,
          filt=None, n_points=None, removed_by=None):
    """THE RANK FUSION, one scalar at a time.  filt: None or a dict with any of deleted (ids), masks (bool [n_masks,
    allow_bits]) with mask_of [nq] (-1 / MAX: none; absent: row 0), labels with lo / hi [nq].  removed_by: a list that
    receives (query, list slot, position among the present entries, id, reason) of every entry removed as inadmissible
    -> (ids, scores, dists or None, counts, unique, dropped, statuses)"""
    f = np.float32
    filt = filt or {}
    nq = ids0.shape[0] if ids0 is not None else ext_ids.shape[0]
    E = 0 if ext_ids is None else ext_ids.shape[1]
    worst = -np.inf if mode == RRF else np.inf
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_scores = np.full((nq, n_out), worst, dtype=np.float32)
    o_dists = None if Q is None else np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, o_unique, o_dropped = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
    o_status = np.zeros(nq, dtype=np.int64)
    deleted = set(int(i) for i in (filt["deleted"] if filt.get("deleted") is not None else ()))
    masks, labels = filt.get("masks"), filt.get("labels")
    for q in range(nq):
        if statuses0 is not None and int(statuses0[q]) != OK:
            o_status[q] = int(statuses0[q])
            continue
        row = None
        if masks is not None:
            m = 0 if filt.get("mask_of") is None else int(filt["mask_of"][q])
            if m not in (-1, MAX):
                if not 0 <= m < len(masks):
                    o_status[q] = ERR_ARG
                    continue
                row = masks[m]
        lo = hi = None
        if filt.get("lo") is not None:
            lo, hi = int(np.broadcast_to(filt["lo"], (nq,))[q]), int(np.broadcast_to(filt["hi"], (nq,))[q])
        lists = []  # (the list's slot of the weights, [(id, score)]): the present entries in order
        if ids0 is not None:
            pool = ids0.shape[1]
            lists.append((0, [(int(ids0[q, j]), None) for j in range(pool)
                              if (int(ids0[q, j]) != MAX if counts0 is None else j < min(int(counts0[q]), pool))]))
        for e in range(E):
            W = ext_ids.shape[2]
            lists.append((1 + e, [(int(ext_ids[q, e, j]), None if ext_scores is None else ext_scores[q, e, j]) for j in range(W)
                                  if (int(ext_ids[q, e, j]) != MAX if ext_counts is None else j < min(int(ext_counts[q][e]), W))]))
        if n_points is not None and any(i >= n_points for _, entries in lists for i, _ in entries):
            o_status[q] = ERR_ARG
            continue
        if Q is not None and any(x != x for x in Q[q].tolist()):
            o_status[q] = ERR_NAN_INPUT
            continue
        effective, dropped = [], 0
        for slot, entries in lists:
            kept = []
            for pos, (i, x) in enumerate(entries):
                if not _admissible(i, deleted, row, labels, lo, hi):
                    dropped += 1
                    if removed_by is not None:
                        reason = "deleted" if i in deleted else \
                            "mask" if row is not None and not _admissible(i, (), row, None, None, None) else "label"
                        removed_by.append((q, slot, pos, i, reason))
                    continue
                if any(i == k for k, _ in kept):
                    continue
                kept.append((i, x))
            effective.append((slot, kept))
        o_dropped[q] = dropped
        cand = []
        for _, kept in effective:
            for i, _ in kept:
                if i not in cand:
                    cand.append(i)
        o_unique[q] = len(cand)
        scored = []
        with np.errstate(all="ignore"):
            for c in cand:
                s = None
                if mode == RRF:
                    for slot, kept in effective:
                        for r, (i, _) in enumerate(kept):
                            if i == c:
                                w = f(1.0) if weights is None else f(weights[q, slot])
                                t = f(w / f(rank_constant + r + 1))
                                s = t if s is None else f(s + t)
                else:
                    if Q is not None:
                        x = f(dist(Q[q], np.array([c], dtype=np.uint32))[0])
                        s = x if weights is None else f(f(weights[q, 0]) * x)
                    for slot, kept in effective:
                        if slot == 0:
                            continue
                        x = f(0.0) if absent is None else f(absent[slot - 1])
                        for i, sc in kept:
                            if i == c:
                                x = f(sc)
                        p = x if weights is None else f(f(weights[q, slot]) * x)
                        s = p if s is None else f(s + p)
                if s is not None and s == s:
                    scored.append((s, c))
        taken = 0
        while scored and taken < n_out:  # the best under the mode's compare, equal scores (-0 == +0) to the lower id
            best = 0
            for k in range(1, len(scored)):
                ahead = scored[k][0] > scored[best][0] if mode == RRF else scored[k][0] < scored[best][0]
                if ahead or (scored[k][0] == scored[best][0] and scored[k][1] < scored[best][1]):
                    best = k
            s, i = scored.pop(best)
            o_ids[q, taken], o_scores[q, taken] = i, s
            if Q is not None:
                o_dists[q, taken] = f(dist(Q[q], np.array([i], dtype=np.uint32))[0])
            taken += 1
        o_counts[q] = taken
    return o_ids, o_scores, o_dists, o_counts, o_unique, o_dropped, o_status


def synthetic_filter(kind, seed, nq=NQ, span=ID_SPAN):
    """the filter of a synthetic call -> None, or the dict naive takes: about a tenth of the ids deleted; N_MASKS rows of
    ALLOW_BITS bits, each about two thirds set, mask_of over the rows and -1 (query 9: a row the set does not have); labels
    0 .. 5 for the first LABEL_LEN ids, lo / hi per query (query 10: lo > hi; query 11: the range [0, 0], which the ids
    beyond the column fall into)"""
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    filt = {}
    if kind in ("deleted", "both"):
        filt["deleted"] = np.sort(rng.permutation(span)[:span // 10]).astype(np.uint32)
    if kind in ("set", "both"):
        filt["masks"] = rng.random((N_MASKS, ALLOW_BITS)) < 0.66
        mo = rng.integers(-1, N_MASKS, nq)
        mo[4], mo[5] = 0, 1  # (real rows: the planted queries 4 and 5 have something to remove)
        mo[9] = N_MASKS + 4
        filt["mask_of"] = mo
    if kind in ("range", "both"):
        filt["labels"] = rng.integers(0, 6, LABEL_LEN).astype(np.uint32)
        lo = rng.integers(0, 3, nq)
        hi = lo + rng.integers(0, 4, nq)
        lo[4], hi[4], lo[5], hi[5] = 1, 2, 2, 4
        lo[10], hi[10] = 3, 2
        lo[11], hi[11] = 0, 0
        filt["lo"], filt["hi"] = lo.astype(np.uint32), hi.astype(np.uint32)
    return filt


def inadmissible_ids(filt, q, span=ID_SPAN):
    """ids below `span` that query q's filter removes (empty without a filter)"""
    if not filt:
        return []
    deleted = set(int(i) for i in (filt["deleted"] if filt.get("deleted") is not None else ()))
    row = None
    if filt.get("masks") is not None:
        m = int(filt["mask_of"][q])
        if 0 <= m < len(filt["masks"]):
            row = filt["masks"][m]
    lo = hi = None
    if filt.get("lo") is not None:
        lo, hi = int(filt["lo"][q]), int(filt["hi"][q])
    return [i for i in range(span) if not _admissible(i, deleted, row, filt.get("labels"), lo, hi)]


def synthetic(p0, E, W, with_counts, seed, filt=None):
    """NQ queries: a dense list of p0 ids (p0 == 0: none) and E external lists of W, ids below ID_SPAN, external scores on
    a grid of quarters (a few NaN and +inf), and the queries' rows (element 0: the row of table_dist).  The planted queries:
      0  pads only (counts 0, or every id the pad)         1  the lists identical (as far as their widths go)
      2  the lists disjoint (RRF ties: the id decides)      3  one id twice inside a list, next to each other and apart
      4  an inadmissible entry at rank 1 of every list      5  every entry inadmissible
      6  a failed dense status                              7  an id equal to the length
      8  a NaN in the query's row                           9  (the filter's: a mask_of beyond n_masks)
      10 (the filter's: lo > hi)                            11 ragged counts with a 0 / pads at the front, middle and end
    and the rest ragged at random, their rows over the table rows that hold NaN and +inf.  Queries 4 and 5 need `filt` (the
    synthetic filter of the call) and are ordinary without one.
    -> Q [NQ, 2], ids0 [NQ, p0] or None, counts0, statuses0 [NQ], ext_ids [NQ, E, W] or None, ext_scores, ext_counts"""
    rng = np.random.default_rng(seed)
    widths = ([p0] if p0 else []) + [W] * E
    total = sum(widths)
    flat = rng.integers(0, ID_SPAN, (NQ, total)).astype(np.uint32)
    counts = np.stack([rng.integers(0, w + 1, NQ) for w in widths], axis=1).astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    Q = np.zeros((NQ, 2), dtype=np.float32)
    Q[:, 0] = rng.integers(0, 40, NQ)
    Q[N_PLANTED:, 0] = rng.integers(36, MC.N_TABLE_ROWS, NQ - N_PLANTED)
    statuses = np.zeros(NQ, dtype=np.int64)
    one = rng.permutation(ID_SPAN)[:max(widths)].astype(np.uint32)
    for l, w in enumerate(widths):
        flat[1, starts[l]:starts[l] + w] = one[:w]
    flat[2] = rng.permutation(ID_SPAN)[:total]
    for q in (1, 2, 3, 4, 5, 7, 8, 9, 10):
        counts[q] = widths
    counts[0] = 0
    w0 = widths[0]
    flat[3, :w0] = rng.permutation(ID_SPAN)[:w0]
    if w0 >= 3:
        flat[3, 1] = flat[3, 0]
        flat[3, w0 - 1] = flat[3, 0]
    bad4, bad5 = inadmissible_ids(filt, 4), inadmissible_ids(filt, 5)
    if bad4:
        for l in range(len(widths)):
            flat[4, starts[l]] = bad4[(3 * l) % len(bad4)]
    if bad5:
        flat[5] = rng.choice(np.array(bad5, dtype=np.uint32), total)
    if p0:
        statuses[6] = ERR_OVERFLOW
    flat[7, total - 1] = ID_SPAN
    Q[8, 1] = np.nan
    counts[11, 0] = 0
    counts[11, -1] = max(widths[-1] - 1, 0)
    if not with_counts:
        absent = rng.random((NQ, total)) < 0.25
        absent[1:11] = False
        absent[0] = True
        for l, w in enumerate(widths):
            absent[11, starts[l]] = absent[11, starts[l] + w // 2] = absent[11, starts[l] + w - 1] = True
        if widths[-1] > 3:
            absent[11, starts[-2] + 1] = False  # (something is left)
        flat[absent] = MAX
        counts = None
    ids0 = np.ascontiguousarray(flat[:, :p0]) if p0 else None
    ext = np.ascontiguousarray(flat[:, p0:].reshape(NQ, E, W)) if E else None
    scores = None
    if E:
        scores = (rng.integers(-8, 9, (NQ, E, W)).astype(np.float32) * np.float32(0.25))
        wild = rng.random((NQ, E, W))
        scores[N_PLANTED:][wild[N_PLANTED:] < 0.06] = np.nan
        scores[N_PLANTED:][wild[N_PLANTED:] > 0.95] = np.inf
    c0 = counts[:, 0].copy() if (counts is not None and p0) else None
    ce = np.ascontiguousarray(counts[:, (1 if p0 else 0):]) if (counts is not None and E) else None
    return Q, ids0, c0, (statuses if p0 else None), ext, scores, ce


def weights_of(kind, E, seed):
    """None; all 1.0 (bit for bit the same answer in BOTH modes: 1.0f * x is x, and 1.0f is RRF's numerator without
    weights); negative, zero and fractional weights, a +inf weight in query 12 and a NaN weight in query 13"""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((NQ, 1 + E), dtype=np.float32)
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([-1.5, -1.0, 0.0, 0.5, 1.0, 2.0], dtype=np.float32), (NQ, 1 + E))
    w[12, 0] = np.inf
    w[13, E] = np.nan
    return np.ascontiguousarray(w, dtype=np.float32)


def absent_of(E, seed):
    """the scores of a candidate an external list does not hold: None on even seeds, values on the quarters' grid otherwise"""
    if E == 0 or seed % 2 == 0:
        return None
    return (np.random.default_rng(seed).integers(-4, 5, E).astype(np.float32) * np.float32(0.5))


def filters_args(filt):
    """the dict naive takes -> the keyword arguments of hnsw_rs_amd.hybrid.filters_of"""
    filt = filt or {}
    return dict(deleted=filt.get("deleted"), masks=filt.get("masks"), mask_of=filt.get("mask_of"), labels=filt.get("labels"),
                lo=filt.get("lo"), hi=filt.get("hi"))


def exercised(dense_ids, dense_counts, ext_ids, ext_counts, fused, removed_by=None, filtered=False):
    """what keeps the search comparison from passing vacuously, asked of the ORACLE's dense lists [nq, pool], the external
    lists [nq, E, W] and their fusion `fused` (naive's tuple) alone -> a dict of booleans: some answer holds an id only an
    external list proposed; some answer holds an id both proposed; some pair of neighbouring hits ties on score and is
    ordered by id; and, filtered, an external entry removed by each of deleted / mask / label, and a returned hit that
    stands behind a removed entry of its list"""
    nq = dense_ids.shape[0]
    ids, scores, counts = fused[0], fused[1], fused[3]
    out = dict(ext_only=False, both=False, tie=False)
    for q in range(nq):
        dense = set(dense_ids[q, :dense_counts[q]].tolist())
        ext = set()
        for e in range(ext_ids.shape[1]):
            k = ext_ids.shape[2] if ext_counts is None else int(ext_counts[q, e])
            ext |= set(int(i) for i in ext_ids[q, e, :k] if int(i) != MAX)
        hits = [int(i) for i in ids[q, :counts[q]]]
        out["ext_only"] |= any(i in ext and i not in dense for i in hits)
        out["both"] |= any(i in ext and i in dense for i in hits)
        out["tie"] |= any(scores[q, a] == scores[q, a + 1] and hits[a] < hits[a + 1] for a in range(len(hits) - 1))
    if filtered:
        reasons = {r for (_, slot, _, _, r) in removed_by if slot >= 1}
        out.update(by_deleted="deleted" in reasons, by_mask="mask" in reasons, by_label="label" in reasons)
        shifted = False
        for (q, slot, pos, _, _) in removed_by:
            if slot == 0:
                continue
            e = slot - 1
            k = ext_ids.shape[2] if ext_counts is None else int(ext_counts[q, e])
            present = [int(i) for i in ext_ids[q, e, :k] if int(i) != MAX]
            shifted |= any(i in set(int(x) for x in ids[q, :counts[q]]) for i in present[pos + 1:])
        out["shifted"] = shifted
    return out


def assert_equal(got, want, what=""):
    """ids, score bits, distance bits, counts, unique, dropped and statuses, exactly"""
    for k, name in enumerate(("ids", "scores", "dists", "counts", "unique", "dropped", "statuses")):
        if k >= len(got) or got[k] is None or want[k] is None:
            assert k >= len(got) or (got[k] is None) == (want[k] is None) or name == "dists", "%s: %s missing" % (what, name)
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32)
        assert g.shape == w.shape, "%s: %s have shapes %s and %s" % (what, name, g.shape, w.shape)
        bad = np.nonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differ for queries %s: got %s want %s" % (what, name, bad[:5], g[bad[:2]], w[bad[:2]])
