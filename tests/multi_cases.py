"""What the multi-vector search tests share (tests/test_multi_host.py, tests/test_gpu_multi.py): a plain-loop restatement
of THE FUSION of include/hnsw_mi355x.h, written independently of hnsw_rs_amd.multi.fuse_lists (scalar float32 arithmetic,
one candidate at a time, no numpy sorting), a synthetic distance and the synthetic candidate lists of the sweep.  A
helper of the tests, no tests of its own."""
import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG, ERR_OVERFLOW = 0, -2, -8, -11
SUM, MIN = 0, 1
NQ = 12        # queries per synthetic call; the first N_PLANTED are the planted ones
N_PLANTED = 9
ID_SPAN = 300  # the synthetic lists draw their ids below this (the "index length" of the host sweep)
SHAPES = [(T, pool) for T in (1, 2, 3, 16) for pool in (1, 16, 64, 256) if T * pool <= 256]


def n_outs(pool):
    return sorted({1, min(10, pool), pool})


def naive(Q, weights, mode, ids_in, counts, statuses, dist, n_out, n_points=None):
    """THE FUSION, one scalar at a time -> (ids, scores, counts, unique, statuses)"""
    f = np.float32
    nq, T, pool = ids_in.shape
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, o_unique = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        first = [int(statuses[q][t]) for t in range(T) if int(statuses[q][t]) != OK] if statuses is not None else []
        if first:
            o_status[q] = first[0]
            continue
        cand = []
        for t in range(T):
            for j in range(pool):
                i = int(ids_in[q, t, j])
                here = i != MAX if counts is None else j < min(int(counts[q][t]), pool)
                if here and i not in cand:
                    cand.append(i)
        if n_points is not None and any(i >= n_points for i in cand):
            o_status[q] = ERR_ARG
            continue
        if any(x != x for t in range(T) for x in Q[q, t].tolist()):
            o_status[q] = ERR_NAN_INPUT
            continue
        o_unique[q] = len(cand)
        scored = []
        with np.errstate(all="ignore"):
            for i in cand:
                s = None
                for t in range(T):
                    p = f(dist(Q[q, t], np.array([i], dtype=np.uint32))[0])
                    if weights is not None:
                        p = f(f(weights[q, t]) * p)
                    if mode == SUM:
                        s = p if s is None else f(s + p)
                    else:
                        s = f(np.inf) if s is None else s
                        if p < s:
                            s = p
                if s == s:
                    scored.append((s, i))
        taken = 0
        while scored and taken < n_out:  # the smallest under f32 <, equal scores (-0 == +0) to the lower id
            best = 0
            for k in range(1, len(scored)):
                if scored[k][0] < scored[best][0] or (scored[k][0] == scored[best][0] and scored[k][1] < scored[best][1]):
                    best = k
            s, i = scored.pop(best)
            o_ids[q, taken], o_scores[q, taken] = i, s
            taken += 1
        o_counts[q] = taken
    return o_ids, o_scores, o_counts, o_unique, o_status


N_TABLE_ROWS = 48


def table_dist(seed=5):
    """a synthetic distance for the host sweep: a vector names a row of a table in its element 0, and its distance to id i
    is table[row, i] -- values on a grid of quarters so that scores tie, zeros, and in the rows from 40 on NaNs and +inf"""
    rng = np.random.default_rng(seed)
    tab = rng.integers(0, 12, (N_TABLE_ROWS, ID_SPAN + 1)).astype(np.float32) * np.float32(0.25)
    wild = rng.random((8, ID_SPAN + 1))
    tab[40:][wild < 0.10] = np.nan
    tab[40:][wild > 0.93] = np.inf

    def dist(q_row, ids):
        return tab[int(q_row[0])][np.asarray(ids, dtype=np.int64)]
    return dist


def synthetic(T, pool, with_counts, seed):
    """NQ queries of T lists of `pool` ids below ID_SPAN, with their vectors (element 0: the row of table_dist).  The
    planted queries:
      0  pads only (counts 0, or every id the pad)        1  the T lists identical; counts above pool
      2  the T lists disjoint                              3  one id twice inside a list, next to each other and apart
      4  failed statuses on vector 0 and on vector T-1     5  a failed status on vector T-1 alone
      6  an id equal to the length                         7  a NaN element in the last vector
      8  pads at the front, in the middle and at the end / ragged counts with a 0
    and the rest ragged at random, their vectors over the table rows that hold NaN and +inf.
    -> Q [NQ, T, 2], ids [NQ, T, pool], counts [NQ, T] (None without), statuses [NQ, T]"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ID_SPAN, (NQ, T, pool)).astype(np.uint32)
    counts = rng.integers(0, pool + 1, (NQ, T)).astype(np.uint32)
    statuses = np.zeros((NQ, T), dtype=np.int64)
    Q = np.zeros((NQ, T, 2), dtype=np.float32)
    Q[:, :, 0] = rng.integers(0, 40, (NQ, T))
    Q[N_PLANTED:, :, 0] = rng.integers(36, N_TABLE_ROWS, (NQ - N_PLANTED, T))
    one = rng.permutation(ID_SPAN)[:pool].astype(np.uint32)
    ids[1] = one[None, :]
    ids[2] = rng.permutation(ID_SPAN)[:T * pool].reshape(T, pool)
    counts[0] = 0
    counts[1] = pool + 3
    counts[2] = counts[3] = counts[6] = counts[7] = pool
    ids[3, 0] = rng.permutation(ID_SPAN)[:pool]
    if pool >= 3:
        ids[3, 0, 1] = ids[3, 0, 0]
        ids[3, 0, pool - 1] = ids[3, 0, 0]
    statuses[4, 0], statuses[4, T - 1] = (ERR_NAN_INPUT, ERR_OVERFLOW) if T > 1 else (ERR_OVERFLOW, ERR_OVERFLOW)
    statuses[5, T - 1] = ERR_OVERFLOW
    ids[6, T - 1, pool - 1] = ID_SPAN
    Q[7, T - 1, 1] = np.nan
    counts[8, 0] = 0
    counts[8, T - 1] = max(pool - 1, 0)
    if not with_counts:
        absent = rng.random((NQ, T, pool)) < 0.25
        absent[1:8] = False
        absent[0] = True
        absent[8, :, 0] = absent[8, :, pool // 2] = absent[8, :, pool - 1] = True
        if pool > 1:
            absent[8, 0, 1 if pool > 3 else 0] = False  # (something is left)
        ids[absent] = MAX
        counts = None
    return Q, ids, counts, statuses


WEIGHT_KINDS = ("none", "ones", "mixed")


def weights_of(kind, T, seed):
    """None; all 1.0 (bit for bit the same answer); negative, zero and fractional weights, a +inf weight in query 10 and a
    NaN weight in query 11"""
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((NQ, T), dtype=np.float32)
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([-1.5, -1.0, 0.0, 0.5, 1.0, 2.0], dtype=np.float32), (NQ, T))
    w[10, 0] = np.inf
    w[11, T - 1] = np.nan
    return np.ascontiguousarray(w, dtype=np.float32)


def near_far_queries(stored, T, nq, seed, noise=0.02):
    """nq queries of T vectors over the stored rows: the first half NEAR -- one stored row plus small noise per vector, so
    the T lists overlap -- the second half FAR -- T unrelated stored rows, a little noise on each -> [nq, T, dim]"""
    rng = np.random.default_rng(seed)
    n, d = stored.shape
    half = nq // 2
    base = rng.choice(n, half, replace=False)
    near = stored[base][:, None, :] + rng.normal(0, noise, (half, T, d)).astype(np.float32)
    far = stored[rng.integers(0, n, (nq - half, T))] + rng.normal(0, noise / 4, (nq - half, T, d)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([near, far]), dtype=np.float32)


def exercised(c_ids, c_counts, fused_ids, T, pool, nq):
    """what keeps the search comparison from passing vacuously, asked of the ORACLE's lists [nq * T, pool] and their
    fusion alone -> (a near query has unique < T * pool, a far query has unique > pool, some query's answer holds an id
    that at least one of its lists misses)"""
    lists = [[set(c_ids[q * T + t, :c_counts[q * T + t]].tolist()) for t in range(T)] for q in range(nq)]
    uniq = [len(set().union(*l)) for l in lists]
    overlap = any(u < T * pool for u in uniq[:nq // 2])
    spread = any(u > pool for u in uniq[nq // 2:])
    fill = any(any(int(i) not in l for l in lists[q]) for q in range(nq) for i in fused_ids[q] if int(i) != MAX)
    return overlap, spread, fill


def assert_fused_equal(got, want, what=""):
    """ids, score bits, counts, unique and statuses, exactly"""
    for k, name in enumerate(("ids", "scores", "counts", "unique", "statuses")):
        if k >= len(got) or got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32)
        assert g.shape == w.shape, "%s: %s have shapes %s and %s" % (what, name, g.shape, w.shape)
        bad = np.nonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differ for queries %s: got %s want %s" % (what, name, bad[:5], g[bad[:2]], w[bad[:2]])
