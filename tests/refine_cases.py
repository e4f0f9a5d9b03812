"""Refined search (include/hnsw_mi355x.h, "refined search"): a second, deliberately plain restatement of THE REFINEMENT
-- Python loops with one np.float32 operation per step, nothing shared with hnsw_rs_amd.refine.refine_lists -- and the
tables and candidate lists the host and the GPU tests share.  No GPU, no library call."""
import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG, ERR_OVERFLOW = 0, -2, -8, -11
F32, F16 = 0, 1
NP_DTYPE = {F32: np.float32, F16: np.float16}
DTYPES = (F32, F16)

# ---- the planted rows of a table (make_table) and the planted queries of a case (make_case) ------------------------------
ROW_TWINS = (0, 1, 2)  # three equal rows: equal distances, ranked by id
ROW_ZEROS = 3          # +0 and -0 alternating
ROW_HIT = 4            # query Q_HIT is this row: distance +0
ROW_BIG = 5            # the dtype's largest finite values (f32: 3e38, whose square overflows: distance +inf)
ROW_INF = 6            # +inf in element 0 (only a table handed to the _device call can hold it): NaN against Q_INF
ROW_SUB = 7            # subnormals of the dtype
ROW_MAX = 8            # f16: +-65504
N_PLANTED_ROWS = 9
Q_FAILED, Q_BEYOND, Q_NAN, Q_TWINS, Q_HIT, Q_BIG, Q_EMPTY, Q_ZEROS, Q_INF, Q_LONG = range(10)
N_PLANTED = 10


def widen(table):
    return np.asarray(table).astype(np.float32)  # (exact for float16)


def make_table(rows, full_dim, dtype, seed, with_inf=True):
    """rows x full_dim of float32 or float16: normal values, and the planted rows above.  with_inf False: ROW_INF is an
    ordinary row (what hnsw_row_table_write accepts)"""
    assert rows >= 2 * N_PLANTED_ROWS
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((rows, full_dim)).astype(np.float32).astype(NP_DTYPE[dtype])
    e = np.arange(full_dim)
    sign = np.where(e % 2 == 0, 1.0, -1.0).astype(np.float32)
    t[1] = t[0]
    t[2] = t[0]
    t[ROW_ZEROS] = (0.0 * sign).astype(t.dtype)  # (+0, -0, +0, ...)
    if dtype == F32:
        t[ROW_BIG] = np.float32(3e38) * sign
        t[ROW_SUB] = (np.float32(1e-40) * (1 + e % 7) * sign).astype(np.float32)
        t[ROW_MAX] = np.float32(65504.0) * sign
    else:
        t[ROW_BIG] = (np.float32(65504.0) * sign).astype(np.float16)
        t[ROW_SUB] = ((1 + e % 1023).astype(np.uint16) | np.where(e % 2 == 0, 0, 0x8000).astype(np.uint16)).view(np.float16)
        t[ROW_MAX] = (np.float32(-65504.0) * sign).astype(np.float16)
    if with_inf:
        t[ROW_INF, 0] = np.inf
    return t


def make_case(nq, pool, table, with_counts, seed):
    """-> Qfull [nq, full_dim], ids [nq, pool], counts [nq] or None, statuses [nq]: the planted queries first, random ones
    (ids with repeats, counts from 0 to pool, or pads sprinkled in) behind them"""
    assert nq >= N_PLANTED
    rows, full_dim = table.shape
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, full_dim)).astype(np.float32)
    ids = rng.integers(N_PLANTED_ROWS, rows, size=(nq, pool)).astype(np.uint32)
    counts = rng.integers(0, pool + 1, size=nq).astype(np.uint32)
    statuses = np.zeros(nq, dtype=np.int64)
    pads = rng.random((nq, pool)) < 0.2
    counts[:N_PLANTED] = pool
    pads[:N_PLANTED] = False
    statuses[Q_FAILED] = ERR_OVERFLOW
    ids[Q_BEYOND, pool - 1] = rows            # the first id that is not the table's
    Q[Q_NAN, full_dim // 2] = np.nan
    ids[Q_TWINS] = np.array(ROW_TWINS[::-1], dtype=np.uint32)[np.arange(pool) % 3]  # 2, 1, 0, 2, ...: twins AND duplicate ids
    Q[Q_HIT] = widen(table[ROW_HIT])
    ids[Q_HIT, pool // 2] = ROW_HIT
    ids[Q_BIG, 0] = ROW_BIG
    if table.dtype == np.float16:
        Q[Q_BIG, 0] = np.float32(-3e38)       # (no f16 row is large enough alone: every distance of the query is +inf)
    counts[Q_EMPTY] = 0
    pads[Q_EMPTY] = True
    Q[Q_ZEROS] = np.float32(-0.0)
    ids[Q_ZEROS, :2] = (ROW_SUB, ROW_MAX)[:pool]  # against zeros the subnormals and +-65504 ARE the distance
    ids[Q_ZEROS, pool - 1] = ROW_ZEROS
    Q[Q_INF, 0] = np.inf                      # not a NaN: the query is served, every distance +inf but ROW_INF's NaN
    ids[Q_INF, pool - 1] = ROW_SUB
    ids[Q_INF, 0] = ROW_INF
    ids[Q_LONG, pool // 3] = ROW_MAX
    counts[Q_LONG] = pool + 5                 # a count beyond the pool is the pool
    if with_counts:
        return Q, ids, counts, statuses
    ids[pads] = MAX
    return Q, ids, None, statuses


def naive(Qfull, ids_in, counts, statuses, table, n_out):
    """THE REFINEMENT, one np.float32 operation per step -> ids, dists, counts, statuses"""
    nq, pool = ids_in.shape
    rows, full_dim = table.shape
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64)
    wide = widen(table)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            if statuses is not None and int(statuses[q]) != OK:
                o_status[q] = int(statuses[q])
                continue
            entries = []
            for j in range(pool):
                if counts is not None:
                    if j >= min(int(counts[q]), pool):
                        continue
                elif int(ids_in[q, j]) == MAX:
                    continue
                entries.append(int(ids_in[q, j]))
            if any(i >= rows for i in entries):
                o_status[q] = ERR_ARG
                continue
            if any(x != x for x in Qfull[q]):
                o_status[q] = ERR_NAN_INPUT
                continue
            keyed = []
            for pos, i in enumerate(entries):
                s = np.float32(0.0)
                for e in range(full_dim):
                    t = np.float32(wide[i, e] - Qfull[q, e])
                    s = np.float32(s + np.float32(t * t))
                d = np.float32(np.sqrt(s))
                if d != d:
                    continue
                keyed.append((int(d.view(np.uint32)), i, pos, d))
            keyed.sort(key=lambda k: k[:3])
            for r, k in enumerate(keyed[:n_out]):
                o_ids[q, r], o_dists[q, r] = k[1], k[3]
            o_counts[q] = min(len(keyed), n_out)
    return o_ids, o_dists, o_counts, o_status


def assert_refined_equal(got, want, what):
    """ids, distance BITS, counts and statuses (got may stop short: what a caller did not ask for)"""
    names = ("ids", "dists", "counts", "statuses")
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if names[k] == "dists":
            g, w = np.ascontiguousarray(g, dtype=np.float32).view(np.uint32), np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
        else:
            g, w = g.astype(np.int64), w.astype(np.int64)
        bad = np.argwhere(g.reshape(w.shape) != w)
        assert bad.size == 0, "%s: %s differ at %d places, first %s: %s vs %s" % (
            what, names[k], len(bad), bad[0], g.reshape(w.shape)[tuple(bad[0])], w[tuple(bad[0])])


def check_planted(want, pool, n_out, what):
    """the planted queries did what they are there for (asked of a restatement's answer)"""
    ids, dists, counts, st = want
    assert st[Q_FAILED] == ERR_OVERFLOW and st[Q_BEYOND] == ERR_ARG and st[Q_NAN] == ERR_NAN_INPUT, what
    assert (st != OK).sum() == 3, what
    for q in (Q_FAILED, Q_BEYOND, Q_NAN, Q_EMPTY):
        assert counts[q] == 0 and (ids[q] == MAX).all() and np.isposinf(dists[q]).all(), what
    k = int(counts[Q_TWINS])
    assert k == n_out, what
    assert ids[Q_TWINS, :k].tolist() == sorted([ROW_TWINS[2 - j % 3] for j in range(pool)])[:k], what  # ties by id, copies kept
    assert (dists[Q_TWINS, :k].view(np.uint32) == dists[Q_TWINS, 0].view(np.uint32)).all(), what
    assert ids[Q_HIT, 0] == ROW_HIT and dists[Q_HIT, 0].view(np.uint32) == 0, what
    assert counts[Q_LONG] == n_out and counts[Q_BIG] == n_out, what
    if n_out == pool:
        assert np.isposinf(dists[Q_BIG, pool - 1]), what  # +inf is an ordinary distance, last
        assert counts[Q_INF] == pool - 1 and ROW_INF not in ids[Q_INF].tolist(), what  # a NaN distance is never returned
        assert np.isposinf(dists[Q_INF, :pool - 1]).all() and ids[Q_INF, pool - 1] == MAX, what
        where = ids[Q_ZEROS].tolist().index(ROW_ZEROS)
        assert dists[Q_ZEROS, where].view(np.uint32) == 0, what  # (-0) - (+-0) squared: +0
