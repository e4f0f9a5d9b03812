"""What the document-scoring tests share (tests/test_docs_host.py, tests/test_gpu_docs.py): a plain-loop restatement of THE
DOCUMENT SCORING of include/hnsw_mi355x.h, written independently of hnsw_rs_amd.docs.score_documents (scalar float32
arithmetic, one row at a time, documents as a dict of lists, no numpy sorting or searching), the planted lists of the host
sweep, and the label columns of the GPU shapes.  A helper of the tests, no tests of its own."""
import numpy as np

from tests.late_cases import assert_late_equal, memo  # noqa: F401  (the same seven outputs, compared the same way)

MAX = 0xFFFFFFFF
OK, ERR_NAN_INPUT, ERR_ARG, ERR_OVERFLOW = 0, -2, -8, -11
SUM, SUM_SQ = 0, 1


def naive(Q, mode, docs_in, counts, statuses, dist, labels, deleted, n_out, rows_cap, n_points):
    """THE DOCUMENT SCORING, one scalar at a time -> (doc_labels, scores, best_ids, doc_sizes, counts, n_docs, statuses)"""
    f = np.float32
    nq, T = Q.shape[:2]
    n_in = docs_in.shape[1]
    o_labels = np.zeros((nq, n_out), dtype=np.uint32)
    o_scores = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_best = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_sizes = np.zeros((nq, n_out), dtype=np.uint32)
    o_counts, o_ndocs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    o_status = np.zeros(nq, dtype=np.int64)
    all_ids = np.arange(n_points, dtype=np.uint32)
    gone = set() if deleted is None else set(int(i) for i in deleted)
    rows_of = {}  # label -> its undeleted ids below n_points, ascending
    for i in range(n_points):
        if i in gone:
            continue
        g = int(labels[i]) if labels is not None and i < len(labels) else 0
        rows_of.setdefault(g, []).append(i)
    for q in range(nq):
        if statuses is not None and int(statuses[q]) != OK:
            o_status[q] = int(statuses[q])
            continue
        if any(x != x for t in range(T) for x in Q[q, t].tolist()):
            o_status[q] = ERR_NAN_INPUT
            continue
        cnt = n_in if counts is None else min(int(counts[q]), n_in)
        named = []
        for j in range(cnt):
            g = int(docs_in[q, j])
            if g not in named and g in rows_of:
                named.append(g)
        o_ndocs[q] = len(named)
        scored = []
        # (the distances of vector t to every id, asked once: the loops below read them one at a time)
        D_of = [np.ascontiguousarray(dist(Q[q, t], all_ids), dtype=np.float32) if named else None for t in range(T)]
        with np.errstate(all="ignore"):
            for g in named:
                rows = rows_of[g][:rows_cap]
                s, best = None, None  # best: (distance bits, id)
                for t in range(T):
                    m = f(np.inf)
                    bits = D_of[t].view(np.uint32)
                    for i in rows:
                        D = D_of[t][i]
                        if D != D:
                            continue
                        if D < m:
                            m = D
                        key = (int(bits[i]), i)
                        if best is None or key < best:
                            best = key
                    e = f(m * m) if mode == SUM_SQ else m
                    s = e if s is None else f(s + e)
                if s == s:
                    scored.append((s, g, MAX if best is None else best[1], len(rows_of[g])))
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


# ---- the host sweep: ids below ID_SPAN of tests.multi_cases.table_dist --------------------------------------------------
FEW = np.array([0, 1, 2, 3, 5, 8, 13, 1000, MAX], dtype=np.uint32)  # the labels of the "few" column; 4 and 77 have no row
NQ = 10


def host_columns(id_span, seed):
    """label columns over the ids below id_span: few labels with 0 and UINT32_MAX among them (label 13 is one big
    document: every id from 200 on), the same column cut shorter than the id span (the rest reads 0), and none at all;
    and the deleted ids: every row of label 5, and a few others"""
    rng = np.random.default_rng(seed)
    few = rng.choice(FEW, id_span)
    few[200:] = 13
    deleted = np.unique(np.concatenate([np.flatnonzero(few == 5), rng.integers(0, id_span, 9)])).astype(np.uint32)
    return {"few": few, "short": few[:120].copy(), "none": None}, deleted


def host_lists(T, n_in, with_counts, seed, n_rows=40):
    """NQ lists of n_in labels drawn from FEW and two labels without a row (4, 77), duplicates inside, and their vectors
    (element 0 names a row of table_dist).  Planted:
      0  a count of 0 (without counts: a list of labels without a row)      1  a count above n_in
      2  a failed incoming status                                          3  a NaN vector
      4  one label n_in times                                              5  the labels without a row, and label 5
    -> Q, docs_in, counts (None without), statuses [NQ]"""
    rng = np.random.default_rng(seed)
    pick = np.concatenate([FEW, np.array([4, 77], dtype=np.uint32)])
    docs_in = rng.choice(pick, (NQ, n_in)).astype(np.uint32)
    counts = rng.integers(0, n_in + 1, NQ).astype(np.uint32)
    counts[0], counts[1] = 0, n_in + 3
    counts[2:6] = n_in
    statuses = np.zeros(NQ, dtype=np.int64)
    statuses[2] = ERR_OVERFLOW
    Q = np.zeros((NQ, T, 2), dtype=np.float32)
    Q[:, :, 0] = rng.integers(0, n_rows, (NQ, T))
    Q[6:, :, 0] = rng.integers(36, 48, (NQ - 6, T))  # (the table's rows with NaN and +inf)
    Q[3, T - 1, 1] = np.nan
    docs_in[4] = 13
    docs_in[5] = rng.choice(np.array([4, 77, 5], dtype=np.uint32), n_in)
    if not with_counts:
        docs_in[0] = rng.choice(np.array([4, 77], dtype=np.uint32), n_in)
        counts = None
    return Q, docs_in, counts, statuses


# ---- the GPU shapes: label columns over an index of n ids whose scored rows total what a test asks for ------------------
def column_of_sizes(n, sizes, first_label=1, rest=0):
    """a label column over n ids: document k (label first_label + k) is the next sizes[k] ids, from id 0 on; every id behind
    them has the label `rest` -> labels [n]"""
    lab = np.full(n, rest, dtype=np.uint32)
    at = 0
    for k, s in enumerate(sizes):
        lab[at:at + s] = first_label + k
        at += s
    assert at <= n
    return lab
