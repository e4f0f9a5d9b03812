"""What the diversified-search tests share (tests/test_diverse_host.py, tests/test_gpu_diverse.py): a plain-loop
restatement of THE SELECTION of include/hnsw_mi355x.h, written independently of hnsw_rs_amd.diverse.mmr_select (scalar
float32 arithmetic, one entry at a time, no numpy selection), the synthetic candidate lists of the sweep, and the
clustered rows of the search cases.  A helper of the tests, no tests of its own."""
import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG = 0, -2, -8
POOLS = (1, 32, 33, 64, 65, 200, 256)
LAMBDAS = (0.0, 0.3, 0.5, 1.0)
NQ = 10       # queries per synthetic call; the first N_PLANTED are the planted ones
N_PLANTED = 6
ID_SPAN = 300  # the synthetic lists draw their ids below this, so that pairs repeat


def n_outs(pool):
    return sorted({1, min(10, pool), pool})


def n_queries(pool, n_out):
    """the planted queries alone where the restatements' pair loop is longest (the same properties, less Python time)"""
    return N_PLANTED if pool >= 200 and n_out == pool else NQ


def naive(ids, dists, counts, statuses, pair_dist, lam, n_out, n_points=None):
    """THE SELECTION, one scalar at a time -> (ids, dists, gaps, counts, statuses)"""
    f = np.float32
    nq, pool = ids.shape
    lam = f(lam)
    rest = f(1.0) - lam
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_gaps = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64)
    for q in range(nq):
        if o_status[q] != OK:
            continue
        if counts is None:
            present = [j for j in range(pool) if int(ids[q, j]) != MAX]
        else:
            present = list(range(min(int(counts[q]), pool)))
        if n_points is not None and any(int(ids[q, j]) >= n_points for j in present):
            o_status[q] = ERR_ARG
            continue
        running = {j: f(np.inf) for j in present}
        chosen, taken = [], set()
        with np.errstate(all="ignore"):
            for t in range(n_out):
                if chosen:
                    s = int(ids[q, chosen[-1]])
                    for j in present:
                        if j not in taken:
                            d = f(pair_dist(s, int(ids[q, j])))
                            if d < running[j]:
                                running[j] = d
                best, best_score = None, None
                for j in present:
                    if j in taken:
                        continue
                    m = f(0.0) if t == 0 else running[j]
                    a = f(lam * dists[q, j])
                    b = f(rest * m)
                    score = f(a - b)
                    if score != score:
                        continue
                    if best is None or score < best_score:
                        best, best_score = j, score
                if best is None:
                    break
                o_ids[q, t], o_dists[q, t], o_gaps[q, t] = ids[q, best], dists[q, best], running[best]
                chosen.append(best)
                taken.add(best)
        o_counts[q] = len(chosen)
    return o_ids, o_dists, o_gaps, o_counts, o_status


def synthetic_lists(pool, with_counts, seed, id_span=ID_SPAN, dup_below=200):
    """[NQ][pool] candidate lists, not sorted (the selection is defined by position): ids below id_span, most of them
    below dup_below (where the GPU tests' indexes hold every row twice: pair distances of exactly 0), distances on a
    grid of quarters so that scores tie.  The planted queries:
      0  no entry (count 0, or every id the pad)          1  a count above pool (or: every entry present)
      2  a NaN and a +inf distance (and a -0.0)           3  one id twice, next to each other and far apart
      4  a failed status                                   5  absent entries in the middle / a ragged count
    and the rest ragged at random.  -> ids, dists, counts (None without), statuses"""
    rng = np.random.default_rng(seed)
    ids = np.where(rng.random((NQ, pool)) < 0.8, rng.integers(0, dup_below, (NQ, pool)), rng.integers(0, id_span, (NQ, pool)))
    ids = ids.astype(np.uint32)
    dists = (rng.integers(0, 24, (NQ, pool)).astype(np.float32) * np.float32(0.25))
    counts = rng.integers(0, pool + 1, NQ).astype(np.uint32)
    statuses = np.zeros(NQ, dtype=np.int64)
    counts[0] = 0
    counts[1] = pool + 7
    counts[2] = counts[3] = pool
    if pool >= 3:
        dists[2, pool // 2] = np.nan
        dists[2, pool // 3] = np.inf
        dists[2, 0] = -0.0
        ids[3, 1] = ids[3, 0]
        ids[3, pool - 1] = ids[3, 0]
    statuses[4] = ERR_NAN_INPUT
    counts[4] = pool
    counts[5] = max(pool - 1, 0)
    if not with_counts:
        absent = rng.random((NQ, pool)) < 0.25  # absent entries anywhere, the middle included
        absent[1] = absent[2] = absent[3] = absent[4] = False
        absent[0] = True
        if pool >= 3:
            absent[5, pool // 2] = True
            absent[5, 0] = False
        ids[absent] = MAX
        counts = None
    return ids, dists, counts, statuses


def assert_diverse_equal(got, want, what=""):
    """the first four arrays of both sides -- ids, distance bits, gap bits and counts -- exactly"""
    for k, name in enumerate(("ids", "dists", "gaps", "counts")):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32)
        assert g.shape == w.shape, "%s: %s have shapes %s and %s" % (what, name, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differ for queries %s: got %s want %s" % (what, name, bad[:5], g[bad[:2]], w[bad[:2]])


def grid_pair_dist(seed=5, id_span=ID_SPAN):
    """a synthetic pair distance for the host sweep: |c[a] - c[b]| over coordinates on a grid of eighths -- symmetric,
    exactly 0 for many pairs of different ids"""
    c = np.random.default_rng(seed).integers(0, 40, id_span).astype(np.float32) * np.float32(0.125)
    return lambda a, b: np.float32(abs(c[a] - c[b]))


def clustered_rows(n, d, seed, per_cluster=100, spread=0.01, n_lonely=12, lonely_size=10):
    """Rows in tight clusters of about per_cluster points (centres U[0, 1)^d, members centre + N(0, spread)), so that a
    query's 64 nearest sit in one cluster and its plain top 10 are near-duplicates of one another, and n_lonely small
    groups of lonely_size rows far from every cluster (around centres at 4 + 2 k on every axis), whose members are
    nearer to each other than to anything else.  -> rows [n, d], the lonely groups' centres"""
    rng = np.random.default_rng(seed)
    n_l = n_lonely * lonely_size
    k = max((n - n_l) // per_cluster, 1)
    centres = rng.random((k, d), dtype=np.float32)
    member = rng.integers(0, k, n - n_l)
    rows = centres[member] + rng.normal(0, spread, (n - n_l, d)).astype(np.float32)
    l_centres = (np.float32(4.0) + np.float32(2.0) * np.arange(n_lonely, dtype=np.float32))[:, None] * np.ones((1, d), dtype=np.float32)
    lonely = np.repeat(l_centres, lonely_size, axis=0) + rng.normal(0, spread, (n_l, d)).astype(np.float32)
    rows = np.concatenate([rows, lonely]).astype(np.float32)
    perm = rng.permutation(n)
    return np.ascontiguousarray(rows[perm]), l_centres


def clustered_queries(rows, l_centres, nq, seed, spread=0.01):
    """nq queries: most of them a stored row of a cluster moved a little, the last len(l_centres) at the lonely groups,
    far from every cluster"""
    rng = np.random.default_rng(seed)
    n_far = l_centres.shape[0]
    in_cluster = np.flatnonzero((rows < 2.0).all(axis=1))
    near = rows[rng.choice(in_cluster, nq - n_far, replace=False)]
    Q = np.concatenate([near, l_centres]).astype(np.float32)
    return np.ascontiguousarray(Q + rng.normal(0, spread / 2, Q.shape).astype(np.float32))
