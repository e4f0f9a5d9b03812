"""Boosted search (include/hnsw_mi355x.h, "boosted search"): a second, deliberately plain restatement of THE BOOST --
Python loops with one np.float32 operation per step, nothing shared with hnsw_rs_amd.boost.boost_lists -- and the
attribute tables, candidate lists and weight rows the host and the GPU tests share.  The primitive needs no index, so the
lists are synthetic.  No GPU, no library call."""
import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_ARG, ERR_OVERFLOW = 0, -8, -11
F32, F16 = 0, 1
NP_DTYPE = {F32: np.float32, F16: np.float16}
DTYPES = (F32, F16)
POOLS = (1, 63, 64, 65, 256, 1024)  # the lane-stride edges: one pass less one, one pass, one pass and one, many passes
ATTRS = (1, 2, 31, 32)              # element loads and 16-byte loads of both dtypes, one and many pieces

# ---- the planted rows of a table (make_table) -----------------------------------------------------------------------------
ROW_TWINS = (0, 1, 2)  # three equal rows: with equal distances equal scores, ranked by id
ROW_NEG = 3            # every attribute -1
ROW_POS = 5            # every attribute +1 (a larger id than ROW_NEG: under Q_ZEROS its -0 must not rank before that +0)
ROW_SUB = 6            # subnormals of the dtype
ROW_BIG = 7            # the dtype's largest finite values, alternating in sign
N_PLANTED_ROWS = 8
# attribute 0 of every other row i is (i % 17) - 8: negative, zero and positive, exact in both dtypes

# ---- the planted queries of a case (make_case).  Those marked W need a weight row of their own: with one row shared by
# ---- every query they are ordinary queries
(Q_FAILED,   # an incoming failed status: kept, count 0, padded rows
 Q_BEYOND,   # a present id equal to table_rows: ERR_ARG
 Q_EMPTY,    # count 0 (without counts: every id a pad)
 Q_LONG,     # a count beyond the pool is the pool
 Q_TWINS,    # equal scores: the id decides; every id three times over: equal (score, id), the position decides
 Q_TIES,     # W: every weight 0 and finite distinct distances: every score +0, ids repeat, so (id, position) is the order
             #    and the returned distances show the position
 Q_ZEROS,    # W: w = (-1, -0, -0, ...) and every distance +0: ROW_POS scores -0, ROW_NEG +0; they tie, +0 bits come back
 Q_INFW,     # W: w = (1, -inf, 0, ...): attribute 0 positive -> -inf (first), negative -> +inf (last, returned), zero -> NaN
             #    (never returned)
 Q_NANW,     # W: a NaN weight: every score NaN, count 0, status OK
 Q_W0ZERO,   # W: w[0] = 0 and some distances +inf: 0 * inf is NaN, those entries are dropped
 Q_DINF,     # some distances +inf under a positive w[0] (W: w = (1, 0, ...)): +inf scores, last but returned
 Q_EDGE,     # the subnormal row and the largest values (f32: products overflow; a NaN of +inf - inf is dropped)
 ) = range(12)
N_PLANTED = 12
NQ = N_PLANTED + 1  # the planted queries and a random one


def widen(table):
    return np.asarray(table).astype(np.float32)  # (exact for float16)


def make_table(rows, n_attrs, dtype, seed):
    """rows x n_attrs of float32 or float16: normal values, attribute 0 as above, and the planted rows"""
    assert rows >= 2 * N_PLANTED_ROWS + 17
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((rows, n_attrs)).astype(np.float32).astype(NP_DTYPE[dtype])
    t[:, 0] = (np.arange(rows) % 17 - 8).astype(t.dtype)
    e = np.arange(n_attrs)
    sign = np.where(e % 2 == 0, 1.0, -1.0).astype(np.float32)
    t[1] = t[0]
    t[2] = t[0]
    t[ROW_NEG] = -1
    t[ROW_POS] = 1
    if dtype == F32:
        t[ROW_SUB] = (np.float32(1e-40) * (1 + e % 7) * sign).astype(np.float32)
        t[ROW_BIG] = np.float32(3e38) * sign
    else:
        t[ROW_SUB] = ((1 + e % 1023).astype(np.uint16) | np.where(e % 2 == 0, 0, 0x8000).astype(np.uint16)).view(np.float16)
        t[ROW_BIG] = (np.float32(65504.0) * sign).astype(np.float16)
    return t


def make_case(pool, table, with_counts, per_query, seed, nq=NQ):
    """-> ids [nq, pool], dists [nq, pool], counts [nq] or None, statuses [nq], weights [nq, 1 + A] or [1 + A]: the planted
    queries first, random ones (ids with repeats, counts from 0 to pool, or pads sprinkled into the middle) behind them"""
    assert nq >= N_PLANTED
    rows, n_attrs = table.shape
    rng = np.random.default_rng(seed)
    ids = rng.integers(N_PLANTED_ROWS, rows, size=(nq, pool)).astype(np.uint32)
    dists = (np.abs(rng.standard_normal((nq, pool))) * 10).astype(np.float32)
    counts = rng.integers(0, pool + 1, size=nq).astype(np.uint32)
    statuses = np.zeros(nq, dtype=np.int64)
    pads = rng.random((nq, pool)) < 0.2
    w = rng.standard_normal((nq, 1 + n_attrs)).astype(np.float32)
    w[:, 0] = np.abs(w[:, 0])
    w[rng.random(w.shape) < 0.1] = 0  # (some attributes do not count; a w[0] of zero is legal too)
    counts[:N_PLANTED] = pool
    pads[:N_PLANTED] = False
    every3 = np.arange(pool) % 3
    statuses[Q_FAILED] = ERR_OVERFLOW
    ids[Q_BEYOND, pool - 1] = rows  # the first id that is not the table's
    counts[Q_EMPTY] = 0
    pads[Q_EMPTY] = True
    counts[Q_LONG] = pool + 5
    ids[Q_EDGE, 0] = ROW_BIG
    ids[Q_EDGE, pool - 1] = ROW_SUB
    ids[Q_TWINS] = np.array(ROW_TWINS[::-1], dtype=np.uint32)[every3]  # 2, 1, 0, 2, ...: twins AND duplicate ids
    dists[Q_TWINS] = np.float32(1.5)
    ids[Q_TIES] = (N_PLANTED_ROWS + 2 - every3).astype(np.uint32)
    dists[Q_TIES] = (1 + np.arange(pool)[::-1]).astype(np.float32)  # descending: the order kept is not the distances'
    dists[Q_ZEROS] = np.float32(0.0)
    ids[Q_ZEROS, 0] = ROW_POS
    ids[Q_ZEROS, pool - 1] = ROW_NEG  # (pool 1: the one entry is ROW_NEG)
    dists[Q_W0ZERO, ::2] = np.inf
    dists[Q_DINF, pool // 2:] = np.inf
    w[Q_TIES] = 0
    w[Q_ZEROS] = -0.0
    w[Q_ZEROS, 0] = -1
    w[Q_INFW] = 0
    w[Q_INFW, :2] = (1, -np.inf)
    w[Q_NANW, 1 + (n_attrs - 1) // 2] = np.nan
    w[Q_W0ZERO, 0] = 0
    w[Q_DINF] = 0
    w[Q_DINF, 0] = 1
    if not per_query:
        w = w[N_PLANTED].copy()  # the random query's row, for all of them
        w[0] = max(w[0], np.float32(0.25))
    if with_counts:
        return ids, dists, counts, statuses, w
    ids[pads] = MAX
    return ids, dists, None, statuses, w


def score(w, d, a):
    """the score of one entry: one np.float32 operation per step (NumPy has no fused multiply-add)"""
    s = np.float32(np.float32(w[0]) * np.float32(d))
    for k in range(len(a)):
        p = np.float32(np.float32(w[k + 1]) * np.float32(a[k]))
        s = np.float32(s + p)
    return s


def naive(ids_in, dists_in, counts, statuses, table, weights, n_outs):
    """THE BOOST, entry by entry, for every n_out of `n_outs` (the entries are scored and ranked once, every n_out cuts the
    ranking for itself) -> {n_out: (ids, scores, dists, counts, statuses)}"""
    nq, pool = ids_in.shape
    rows = table.shape[0]
    wide = widen(table)
    weights = np.asarray(weights, dtype=np.float32)
    out = {n: (np.full((nq, n), MAX, dtype=np.uint32), np.full((nq, n), np.inf, dtype=np.float32),
               np.full((nq, n), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.int64))
           for n in n_outs}
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for q in range(nq):
            if statuses is not None and int(statuses[q]) != OK:
                for n in n_outs:
                    out[n][4][q] = int(statuses[q])
                continue
            entries = []
            for j in range(pool):
                if counts is not None:
                    if j >= min(int(counts[q]), pool):
                        continue
                elif int(ids_in[q, j]) == MAX:
                    continue
                entries.append((j, int(ids_in[q, j])))
            if any(i >= rows for _, i in entries):
                for n in n_outs:
                    out[n][4][q] = ERR_ARG
                continue
            w = weights if weights.ndim == 1 else weights[q]
            ranked = []
            for j, i in entries:
                s = score(w, dists_in[q, j], wide[i])
                if s != s:
                    continue
                if s == 0:
                    s = np.float32(0.0)
                ranked.append((float(s), i, j))  # (a float32 is a Python float exactly, and < on them is f32's)
            ranked.sort()
            for n in n_outs:
                o_ids, o_scores, o_dists, o_counts, _ = out[n]
                for r, (s, i, j) in enumerate(ranked[:n]):
                    o_ids[q, r], o_scores[q, r], o_dists[q, r] = i, np.float32(s), dists_in[q, j]
                o_counts[q] = min(len(ranked), n)
    return out


def assert_boosted_equal(got, want, what):
    """ids, score BITS, distance BITS, counts and statuses (got may stop short or hold None: what a caller did not ask for)"""
    names = ("ids", "scores", "dists", "counts", "statuses")
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if names[k] in ("scores", "dists"):
            g, w = np.ascontiguousarray(g, dtype=np.float32).view(np.uint32), np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
        else:
            g, w = g.astype(np.int64), w.astype(np.int64)
        bad = np.argwhere(g.reshape(w.shape) != w)
        assert bad.size == 0, "%s: %s differ at %d places, first %s: %s vs %s" % (
            what, names[k], len(bad), bad[0], g.reshape(w.shape)[tuple(bad[0])], w[tuple(bad[0])])


def check_planted(want, ids_in, dists_in, table, pool, n_out, per_query, what):
    """the planted queries did what they are there for (asked of a restatement's answer)"""
    ids, scores, dists, counts, st = want
    assert st[Q_FAILED] == ERR_OVERFLOW and st[Q_BEYOND] == ERR_ARG and (st != OK).sum() == 2, what
    for q in (Q_FAILED, Q_BEYOND, Q_EMPTY):
        assert counts[q] == 0 and (ids[q] == MAX).all() and np.isposinf(scores[q]).all() and np.isposinf(dists[q]).all(), what
    assert not np.isnan(scores).any(), what
    for q in range(len(ids)):  # ascending by (score, id), padded behind the count, -0 nowhere
        c = int(counts[q])
        assert all((scores[q, a], ids[q, a]) <= (scores[q, a + 1], ids[q, a + 1]) for a in range(c - 1)), what
        assert (ids[q, c:] == MAX).all() and np.isposinf(scores[q, c:]).all() and np.isposinf(dists[q, c:]).all(), what
        assert not (scores[q].view(np.uint32) == 0x80000000).any(), what
    assert counts[Q_LONG] == n_out, what
    k = int(counts[Q_TWINS])
    assert k == n_out and ids[Q_TWINS, :k].tolist() == sorted(ROW_TWINS[2 - j % 3] for j in range(pool))[:k], what
    assert (scores[Q_TWINS, :k].view(np.uint32) == scores[Q_TWINS, 0].view(np.uint32)).all(), what
    if not per_query:
        return
    # every score +0: ascending ids, and within an id the incoming positions ascending, which the distances (descending
    # along the list) show
    k = int(counts[Q_TIES])
    order = sorted((int(ids_in[Q_TIES, j]), j) for j in range(pool))[:n_out]
    assert k == n_out and (scores[Q_TIES, :k].view(np.uint32) == 0).all(), what
    assert ids[Q_TIES, :k].tolist() == [i for i, _ in order], what
    assert dists[Q_TIES, :k].tolist() == [float(dists_in[Q_TIES, j]) for _, j in order], what
    assert counts[Q_NANW] == 0 and st[Q_NANW] == OK, what
    if n_out != pool:
        return
    assert (scores[Q_ZEROS].view(np.uint32) == 0).all() and counts[Q_ZEROS] == pool, what
    assert ids[Q_ZEROS].tolist() == sorted(ids_in[Q_ZEROS].tolist()), what  # a -0 did not jump the queue
    a0 = widen(table)[ids_in[Q_INFW].astype(np.int64), 0]
    n_neg_inf, n_pos_inf = int((a0 > 0).sum()), int((a0 < 0).sum())
    assert counts[Q_INFW] == n_neg_inf + n_pos_inf, what  # inf * 0 is NaN: never returned
    assert np.isneginf(scores[Q_INFW, :n_neg_inf]).all() and np.isposinf(scores[Q_INFW, n_neg_inf:]).all(), what
    assert counts[Q_W0ZERO] == pool // 2 and np.isfinite(dists[Q_W0ZERO, :pool // 2]).all(), what  # 0 * inf dropped
    assert counts[Q_DINF] == pool, what  # +inf is an ordinary score: last, but returned
    assert np.isposinf(scores[Q_DINF, pool // 2:]).all() and np.isfinite(scores[Q_DINF, :pool // 2]).all(), what
