"""What the late-interaction tests share (tests/test_late_host.py, tests/test_gpu_late.py): a plain-loop restatement of
THE LATE INTERACTION of include/hnsw_mi355x.h, written independently of hnsw_rs_amd.late.late_interaction (scalar float32
arithmetic, one candidate at a time, no numpy sorting), the label columns and candidate lists of the GPU sweep, and
assert_late_equal.  A helper of the tests, no tests of its own."""
import numpy as np

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG, ERR_OVERFLOW = 0, -2, -8, -11
SUM, SUM_SQ = 0, 1
NAMES = ("doc_labels", "scores", "best_ids", "doc_sizes", "counts", "n_docs", "statuses")


def naive(Q, mode, ids_in, counts, statuses, dist, labels, n_out, n_points=None):
    """THE LATE INTERACTION, one scalar at a time -> (doc_labels, scores, best_ids, doc_sizes, counts, n_docs, statuses)"""
    f = np.float32
    nq, T, pool = ids_in.shape
    o_labels = np.zeros((nq, n_out), dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_best = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_sizes = np.zeros((nq, n_out), dtype=np.uint32)
    o_counts, o_ndocs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
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
        docs = {}  # label -> its candidates
        for i in cand:
            g = int(labels[i]) if labels is not None and i < len(labels) else 0
            docs.setdefault(g, []).append(i)
        o_ndocs[q] = len(docs)
        scored = []
        with np.errstate(all="ignore"):
            for g, rows in docs.items():
                s, best = None, None  # best: (distance bits, id)
                for t in range(T):
                    m = f(np.inf)
                    for i in rows:
                        D = f(dist(Q[q, t], np.array([i], dtype=np.uint32))[0])
                        if D != D:
                            continue
                        if D < m:
                            m = D
                        key = (int(np.array([D], dtype=np.float32).view(np.uint32)[0]), i)
                        if best is None or key < best:
                            best = key
                    e = f(m * m) if mode == SUM_SQ else m
                    s = e if s is None else f(s + e)
                if s == s:
                    scored.append((s, g, MAX if best is None else best[1], len(rows)))
        taken = 0
        while scored and taken < n_out:  # the smallest under f32 <, equal scores (-0 == +0) to the lower label
            b = 0
            for k in range(1, len(scored)):
                if scored[k][0] < scored[b][0] or (scored[k][0] == scored[b][0] and scored[k][1] < scored[b][1]):
                    b = k
            s, g, row, size = scored.pop(b)
            o_labels[q, taken], o_scores[q, taken], o_best[q, taken], o_sizes[q, taken] = g, s, row, size
            taken += 1
        o_counts[q] = taken
    return o_labels, o_scores, o_best, o_sizes, o_counts, o_ndocs, o_status


def assert_late_equal(got, want, what=""):
    """labels, score bits, best ids, sizes, counts, n_docs and statuses, exactly (an entry of `got` that is None is skipped)"""
    for k, name in enumerate(NAMES):
        if k >= len(got) or got[k] is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
        assert g.shape == w.shape, "%s: %s have shapes %s and %s" % (what, name, g.shape, w.shape)
        bad = np.nonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differ for queries %s: got %s want %s" % (what, name, bad[:5], g[bad[:2]], w[bad[:2]])


def random_case(T, pool, with_counts, seed, id_span, dim=2, n_rows=40):
    """nq = 10 queries of T lists of ids below id_span with duplicates inside and across lists, ragged counts (or pads),
    vectors whose element 0 names a row of tests.multi_cases.table_dist below n_rows; query 0 has no entry
    -> Q, ids, counts (None without), statuses (all OK)"""
    rng = np.random.default_rng(seed)
    nq = 10
    ids = rng.integers(0, id_span, (nq, T, pool)).astype(np.uint32)
    counts = rng.integers(0, pool + 1, (nq, T)).astype(np.uint32)
    counts[1] = pool + 2
    counts[0] = 0
    Q = np.zeros((nq, T, dim), dtype=np.float32)
    Q[:, :, 0] = rng.integers(0, n_rows, (nq, T))
    if not with_counts:
        absent = rng.random((nq, T, pool)) < 0.3
        absent[0], absent[1] = True, False
        ids[absent] = MAX
        counts = None
    return Q, ids, counts, np.zeros((nq, T), dtype=np.int64)


# ---- the GPU sweep: an index of 1500 points whose rows 1400 .. 1499 repeat rows 0 .. 99 ---------------------------------
N = 1500
NQ = 24
N_PLANTED = 12
SHORT = 1300  # the length of the short label column: ids from here on have label 0 under it


def sweep_labels():
    """the label column of the sweep: every id a document of its own (label 10000 + id) but for
      50 .. 99 and their twins 1450 .. 1499   one label per pair of twin rows (5000 + id % 50)
      200 .. 399                              one document (label 7)
      600 .. 619 / 620 .. 639                 the labels 0 and UINT32_MAX
    so that the twins 0 .. 49 / 1400 .. 1449 are documents of their own with equal scores"""
    lab = (10000 + np.arange(N)).astype(np.uint32)
    lab[50:100] = 5000 + np.arange(50)
    lab[1450:1500] = 5000 + np.arange(50)
    lab[200:400] = 7
    lab[600:620] = 0
    lab[620:640] = MAX
    return lab


OWN = np.concatenate([np.arange(0, 50), np.arange(100, 200), np.arange(400, 600), np.arange(640, 1300)])  # 1010 ids


def sweep_lists(stored, T, pool, seed):
    """NQ queries of T lists over the index of the sweep, vectors near stored rows, a stats record per list.  Planted:
      0  no entry (counts 0)                              1  the T lists identical
      2  every entry distinct, every candidate a document of its own (n_docs = T * pool)
      3  every candidate in the one document 200 .. 399    4  an id equal to the length
      5  a NaN vector                                      6  a failed incoming status on the last vector
      7  rows 0 .. 49 next to their twins 1400 .. 1449: two documents with equal scores, the label decides
      8  rows 50 .. 99 next to their twins 1450 .. 1499 under one label: the best row is decided by the id
      9  the labels 0 and UINT32_MAX (600 .. 639)         10  counts above pool
     11  ids from SHORT on (label 0 under the short column) next to ids before it
    and the rest at random with ragged counts.  -> Q, ids, counts, stats [NQ, T, 4]"""
    rng = np.random.default_rng(seed)
    total = T * pool
    twins = np.concatenate([np.arange(100), np.arange(1400, 1500)])
    ids = np.where(rng.random((NQ, T, pool)) < 0.5, rng.choice(twins, (NQ, T, pool)), rng.integers(0, N, (NQ, T, pool)))
    ids = ids.astype(np.uint32)
    counts = rng.integers(0, pool + 1, (NQ, T)).astype(np.uint32)
    counts[:N_PLANTED] = pool
    counts[N_PLANTED::3] = pool
    counts[0] = 0
    ids[1] = ids[1, 0][None, :]
    own = rng.permutation(np.concatenate([OWN, np.arange(1400, 1450)]))  # 1060 ids, a document each
    ids[2] = own[:total].reshape(T, pool)
    ids[3] = rng.integers(200, 400, (T, pool))
    ids[4, T - 1, 0] = N
    a = rng.integers(0, 50, (T, pool))
    ids[7] = np.where(rng.random((T, pool)) < 0.5, a, a + 1400)
    if total >= 2:
        ids[7].reshape(-1)[:2] = (3, 1403)
    b = rng.integers(50, 100, (T, pool))
    ids[8] = np.where(rng.random((T, pool)) < 0.5, b, b + 1400)
    if total >= 2:
        ids[8].reshape(-1)[:2] = (1461, 61)
    ids[9] = rng.integers(600, 640, (T, pool))
    counts[10] = pool + 5
    ids[11] = np.where(rng.random((T, pool)) < 0.5, rng.integers(SHORT, 1400, (T, pool)), rng.integers(400, 600, (T, pool)))
    stats = rng.integers(2 ** 31, 2 ** 32, (NQ, T, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    stats[6, T - 1, 3] = ERR_OVERFLOW & 0xFFFFFFFF
    src = rng.integers(0, N, (NQ, T))
    src[7], src[8] = rng.integers(0, 50, T), rng.integers(50, 100, T)
    Q = stored[src] + rng.normal(0, 0.05, (NQ, T, stored.shape[1])).astype(np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    Q[5, T - 1, stored.shape[1] // 2] = np.nan
    return Q, ids, counts, stats


def memo(dist):
    """dist with its answers kept: the two modes of a case ask for the same distances"""
    kept = {}

    def f(q_row, ids):
        key = (np.asarray(q_row).tobytes(), np.asarray(ids).tobytes())
        if key not in kept:
            kept[key] = np.array(dist(q_row, ids), dtype=np.float32)
        return kept[key]
    return f
