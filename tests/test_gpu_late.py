"""Late-interaction search on the GPU (include/hnsw_mi355x.h, "late-interaction search"), held to the numpy restatement
(hnsw_rs_amd.late.late_interaction; tests/test_late_host.py holds that to a plain loop) over the CPU oracle's distances
(OracleHNSW.distance_batch) and search (OracleHNSW.search_batch).  All comparisons are exact: labels, score BITS, best ids,
sizes, counts, n_docs, counters and statuses.
  1. hnsw_late_interaction_device alone over host-made lists at the pass boundaries of both vector kinds and the table's
     end: one launch and nothing else, guard words, no word unwritten, the planted queries of tests/late_cases.py;
  2. a planted meaning: the query made of a document's own rows finds that document first with score +0;
  3. search_batch_late against the late interaction of the ORACLE's lists, T = 3 and T = 1; a NaN vector, deletions, the
     cosine option, launch accounting;
  4. capture and replay of the primitive and of the chain search -> late interaction on a torch stream.
The indexes are built by the recipe of tests/test_gpu_from_rows.py in a cache of this file's own: these tests set labels,
and the shared ones stay unchanged.  Every test sets the label column it needs."""
import ctypes as C
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import late_cases as LC
from tests import multi_cases as MC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import M, N, SHAPES, capture_and_replay, guarded, kernel_of, unguard, up
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
NQ = 64
T3, POOL, TOPN, EF = 3, 16, 10, 32
QUERY_SEED = 7
# candidate totals at the pass boundaries of both vector kinds (32 and 64 entries a pass) and at the table's end
TOTALS = {1: (1, 1), 31: (1, 31), 32: (2, 16), 33: (3, 11), 63: (3, 21), 64: (2, 32), 65: (1, 65), 1000: (2, 500),
          1024: (32, 32)}
assert N == LC.N


@functools.lru_cache(maxsize=None)
def world(name):
    """an index of 1500 points whose rows 1400 .. 1499 repeat rows 0 .. 99, the oracle holding its graph, and the rows as
    the oracle returns them (tests/test_gpu_from_rows.py::world's recipe; this file's own copy, whose labels change)"""
    kind, d = SHAPES[name]
    vs = rand_vectors(N, d, 61 + d)
    vs[1400:1500] = vs[0:100]
    lv = O.draw_levels(N, M, 61)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(vs, 4, False, levels=lv)
    orc = oracle_from_product(index, vs, lv)
    stored = np.stack([orc.get_vals(i) for i in range(N)]).astype(np.float32)
    stored.setflags(write=False)
    return index, orc, stored, LC.memo(orc.distance_batch)


def summed_stats(stats_in, statuses):
    """the T incoming records of a query as the late interaction leaves them: wrapping sums, its own status"""
    s = (np.asarray(stats_in).astype(np.uint64)[:, :, :3].sum(axis=1) & 0xFFFFFFFF).astype(np.int64)
    return np.concatenate([s, (np.asarray(statuses).astype(np.int64) & 0xFFFFFFFF)[:, None]], axis=1)


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def late_on_device(index, Q, mode, ids, counts, stats, n_out, extras=True):
    import torch
    nq, T, pool = ids.shape
    d_in = (up(Q), up(ids), None if counts is None else up(counts), None if stats is None else up(stats.astype(np.uint32)))
    sizes = {"labels": nq * n_out, "scores": nq * n_out, "best": nq * n_out if extras else 0, "sizes": nq * n_out if extras else 0,
             "counts": nq if extras else 0, "n_docs": nq if extras else 0, "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.late_interaction_device(nq, T, pool, n_out, mode, d_in[0], d_in[1], d_in[2], d_in[3], out["labels"], out["scores"],
                                      out["best"], out["sizes"], out["counts"], out["n_docs"], out["stats"],
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shape = (nq, n_out)
    r = lambda k: None if got[k] is None else got[k].reshape(shape)  # noqa: E731
    return (r("labels"), got["scores"].view(np.float32).reshape(shape), r("best"), r("sizes"), got["counts"], got["n_docs"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4).astype(np.int64)), log


def statuses_of(stats):
    return stats[:, :, 3].astype(np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("total", list(TOTALS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_primitive_alone_is_the_restatement_bit_for_bit(name, total):
    index, orc, stored, dist = world(name)
    labels = LC.sweep_labels()
    index.set_labels(labels)
    index.upload()
    T, pool = TOTALS[total]
    assert T * pool == total
    Q, ids, counts, stats = LC.sweep_lists(stored, T, pool, 100 * total + len(name))
    statuses = statuses_of(stats)
    launches = index.stat("late_launches")
    # with everything: counts, stats and every optional output; n_out small and at its limit
    for mode, n_out in ((H.LATE_SUM, min(10, total)), (H.LATE_SUM_SQ, min(total, 256))):
        what = "%s total=%d mode=%d" % (name, total, mode)
        want = H.late_interaction(Q, mode, ids, counts, statuses, dist, labels, n_out, N)
        # the planted queries do what they are there for (asked of the restatement before the GPU is)
        assert want[6][4] == _lib.ERR_ARG and want[6][5] == _lib.ERR_NAN_INPUT and want[6][6] == _lib.ERR_OVERFLOW
        assert (want[6] != 0).sum() == 3 and want[4][0] == 0 and want[5][0] == 0
        assert want[5][2] == total and want[4][2] == n_out  # every candidate a document of its own, 1024 of them included
        assert want[5][3] == 1 and want[4][3] == 1 and want[0][3, 0] == 7  # one document: padding behind it
        assert want[3][3, 0] == np.unique(ids[3]).size and (want[0][3, 1:] == 0).all()
        assert set(np.unique(want[0][9, :want[4][9]]).tolist()) <= {0, MAX}
        if total >= 2:
            # the twins under different labels: equal scores, the lower label first (rows 3 and 1403 are both candidates)
            k7, s7, l7 = int(want[4][7]), want[1][7].view(np.uint32), want[0][7].astype(np.int64)
            pairs = [(a, b) for a in range(k7) for b in range(a + 1, k7) if l7[b] - l7[a] == 1400]
            assert all(s7[a] == s7[b] and b == a + 1 for a, b in pairs), what
            assert pairs or want[5][7] > n_out, what
            # the twins under one label: with both rows among the candidates the best row is the lower id (61 and 1461 are)
            k8 = int(want[4][8])
            both = want[3][8, :k8] == 2
            assert (want[2][8, :k8][both] < 100).all() and (want[0][8, :k8] < 5050).all() and (want[3][8, :k8] <= 2).all(), what
            assert both.any() or want[5][8] > n_out, what
        got, log = late_on_device(index, Q, mode, ids, counts, stats, n_out)
        assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
        LC.assert_late_equal(got[:6], want, what)
        assert np.array_equal(got[6], summed_stats(stats, want[6])), what
        for q in (0, 4, 5, 6):  # no entry, a bad id, a NaN vector and a failed status: their query alone, padded
            assert got[4][q] == 0 and got[5][q] == 0 and (got[0][q] == 0).all() and np.isposinf(got[1][q]).all()
            assert (got[2][q] == MAX).all() and (got[3][q] == 0).all()
    # bare: no counts (pads mark the absent entries), no stats, no optional output
    bare = ids.copy()
    bare[np.arange(pool)[None, None, :] >= counts[:, :, None]] = MAX
    bare[6] = MAX  # (without statuses query 6 cannot fail: it has no entry instead)
    n_out = min(10, total)
    got, log = late_on_device(index, Q, H.LATE_SUM, bare, None, None, n_out, extras=False)
    want = H.late_interaction(Q, H.LATE_SUM, bare, None, None, dist, labels, n_out, N)
    LC.assert_late_equal((got[0], got[1]), want, name + " bare")
    assert all(g is None for g in got[2:]) and dict(log) == {kernel_of(index): 1}
    assert index.stat("late_launches") == launches + 3 and index.stat("late_calls") == 0


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_the_call_reads_the_label_column_as_of_the_call(name):
    """a column shorter than the index (ids from LC.SHORT on have label 0), then the full one, then another: the second
    and third calls read the new column"""
    index, orc, stored, dist = world(name)
    T, pool = TOTALS[65]
    Q, ids, counts, stats = LC.sweep_lists(stored, T, pool, 5)
    statuses = statuses_of(stats)
    full = LC.sweep_labels()
    answers = []
    for column in (np.concatenate([full[:LC.SHORT], np.zeros(N - LC.SHORT, dtype=np.uint32)]), full, (full // 3).astype(np.uint32)):
        index.set_labels(column)
        want = H.late_interaction(Q, "sum", ids, counts, statuses, dist, column, 10, N)
        got, log = late_on_device(index, Q, "sum", ids, counts, stats, 10)
        LC.assert_late_equal(got[:6], want, name)
        assert dict(log) == {kernel_of(index): 1}
        answers.append(want)
    # (a column that ends early is one that goes on with zeros)
    LC.assert_late_equal(H.late_interaction(Q, "sum", ids, counts, statuses, dist, full[:LC.SHORT], 10, N), answers[0], name)
    assert answers[0][5][11] < answers[1][5][11] and not np.array_equal(answers[0][0], answers[1][0])
    assert not np.array_equal(answers[1][0], answers[2][0])


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_a_handle_that_never_had_labels_has_one_document(kind):
    n, d = 600, 20
    vs = rand_vectors(n, d, 17)
    lv = O.draw_levels(n, M, 5)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(vs, 4, False, levels=lv)
    orc = oracle_from_product(index, vs, lv)
    rng = np.random.default_rng(3)
    T, pool = 3, 21
    ids = rng.integers(0, n, (8, T, pool)).astype(np.uint32)
    Q = np.ascontiguousarray(vs[rng.integers(0, n, (8, T))] + np.float32(0.01))
    want = H.late_interaction(Q, "sum_sq", ids, None, None, orc.distance_batch, None, 4, n)
    assert (want[5] == 1).all() and (want[4] == 1).all() and (want[0] == 0).all()
    got, log = late_on_device(index, Q, "sum_sq", ids, None, None, 4)
    LC.assert_late_equal(got[:6], want, "no labels")
    assert got[6] is None and dict(log) == {kernel_of(index): 1}
    assert (got[3][:, 0] == [np.unique(ids[q]).size for q in range(8)]).all()
    # a column that covers the first half of the ids only: an id at or beyond its length has label 0
    half = (1 + np.arange(n // 2) % 9).astype(np.uint32)
    index.set_labels(half)
    want = H.late_interaction(Q, "sum", ids, None, None, orc.distance_batch, half, 10, n)
    assert (want[5] > 1).all() and ((want[0] == 0) & (want[3] > 1)).any()  # (label 0: the ids of the second half)
    got, log = late_on_device(index, Q, "sum", ids, None, None, 10)
    LC.assert_late_equal(got[:6], want, "half a column")


# ---- 2. a planted meaning ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-16", "f32-100"])
def test_the_query_made_of_a_documents_rows_finds_it_first_with_score_zero(name):
    index, orc, stored, dist = world(name)
    labels = (np.arange(N) // 4).astype(np.uint32)  # documents of 4 consecutive ids
    index.set_labels(labels)
    rng = np.random.default_rng(9)
    docs = rng.choice(np.arange(30, 340), 16, replace=False)  # (clear of the twin rows)
    T, pool = 4, 12
    Q = np.ascontiguousarray(np.stack([stored[4 * x:4 * x + 4] for x in docs]), dtype=np.float32)
    ids = rng.integers(0, N, (16, T, pool)).astype(np.uint32)
    for q, x in enumerate(docs):  # list t holds row t of the document, somewhere; no other list entry is one of its rows
        ids[q][np.isin(ids[q], np.arange(4 * x, 4 * x + 4))] = 0
        ids[q, np.arange(T), rng.integers(0, pool, T)] = 4 * x + np.arange(T)
    for mode in ("sum", "sum_sq"):
        want = H.late_interaction(Q, mode, ids, None, None, dist, labels, 5, N)
        got, _ = late_on_device(index, Q, mode, ids, None, None, 5)
        for r in (want, got):
            assert (r[0][:, 0] == docs).all() and (r[1][:, 0].view(np.uint32) == 0).all()  # score +0
            assert (r[3][:, 0] == 4).all() and (r[2][:, 0] == 4 * docs).all()  # its four rows; the smallest id of them
            assert (r[1][:, 1] > 0).all() and (r[4] == 5).all()
        LC.assert_late_equal(got[:6], want, name + " " + mode)


# ---- 3. the search against the late interaction of the oracle's lists -----------------------------------------------------
def oracle_lists(orc, Q, pool, ef):
    nq, T = Q.shape[:2]
    c = orc.search_batch(Q.reshape(nq * T, -1), pool, ef)
    stats = np.concatenate([np.asarray(c[3]).astype(np.int64), np.zeros((nq * T, 1), dtype=np.int64)], axis=1)
    return np.asarray(c[0]).reshape(nq, T, pool), np.asarray(c[2]).reshape(nq, T), stats.reshape(nq, T, 4)


def search_labels():
    return (np.arange(N) % 61).astype(np.uint32)  # 61 documents of 24 or 25 rows spread over the index


def exercised(c_ids, want, T, pool):
    """what keeps the search comparison from passing vacuously, asked of the ORACLE's lists and their late interaction
    alone -> (some query's lists hold an id twice, some returned document has more than one row among the candidates)"""
    uniq = np.array([np.unique(c_ids[q]).size for q in range(c_ids.shape[0])])
    return bool((uniq < T * pool).any()), bool((want[3] > 1).any())


@pytest.mark.parametrize("name", list(SHAPES))
def test_search_is_the_late_interaction_of_the_oracles_lists(name):
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    for T in (T3, 1):
        Q = MC.near_far_queries(stored, T, NQ, QUERY_SEED)
        c_ids, c_counts, c_stats = oracle_lists(orc, Q, POOL, EF)
        for mode in ("sum", "sum_sq"):
            what = "%s T=%d mode=%s" % (name, T, mode)
            want = H.late_interaction(Q, mode, c_ids, c_counts, None, dist, labels, TOPN, N)
            dup, rows = exercised(c_ids, want, T, POOL)
            assert (dup or T == 1) and rows, "%s: duplicates across vectors %s, documents of several rows %s" % (what, dup, rows)
            got = index.search_batch_late(Q, TOPN, POOL, EF, mode=mode)
            LC.assert_late_equal(got[:6], want, what)
            assert np.array_equal(got[6], summed_stats(c_stats, want[6])), what
            assert (got[4] == np.minimum(got[5], TOPN)).all() and (got[6][:, 3] == 0).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_a_nan_vector_fails_its_query_alone_with_the_query_named(name):
    index, orc, stored, dist = world(name)
    index.set_labels(search_labels())
    Q = MC.near_far_queries(stored, T3, 16, 11)
    Q[3, 2, 1] = np.nan
    with pytest.raises(H.HnswError) as e:
        index.search_batch_late(Q, TOPN, POOL, EF)
    assert e.value.code == _lib.ERR_NAN_INPUT and str(e.value).count("query 3:") == 1, str(e.value)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    labels, scores = np.full((16, TOPN), 7, dtype=np.uint32), np.full((16, TOPN), 3.5, dtype=np.float32)
    best, sizes = np.full((16, TOPN), 7, dtype=np.uint32), np.full((16, TOPN), 7, dtype=np.uint32)
    counts, n_docs, stats = np.full(16, 9, dtype=np.uint32), np.full(16, 9, dtype=np.uint32), np.zeros((16, 4), dtype=np.int32)
    L = _lib.lib()
    rc = L.hnsw_search_batch_late(index._h, Q.ctypes.data_as(f32p), 16, T3, 0, TOPN, POOL, EF, labels.ctypes.data_as(u32p),
                                  scores.ctypes.data_as(f32p), best.ctypes.data_as(u32p), sizes.ctypes.data_as(u32p),
                                  counts.ctypes.data_as(u32p), n_docs.ctypes.data_as(u32p),
                                  C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)))
    assert rc == _lib.ERR_NAN_INPUT and L.hnsw_last_error().startswith(b"query 3:")
    assert counts[3] == 0 and n_docs[3] == 0 and (labels[3] == 0).all() and np.isposinf(scores[3]).all()
    assert (best[3] == MAX).all() and (sizes[3] == 0).all() and stats[3, 3] == _lib.ERR_NAN_INPUT
    good = np.delete(np.arange(16), 3)  # every other row is filled in
    want = index.search_batch_late(Q[good], TOPN, POOL, EF)
    assert np.array_equal(labels[good], want[0]) and np.array_equal(scores[good].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(best[good], want[2]) and np.array_equal(sizes[good], want[3])
    assert np.array_equal(counts[good], want[4]) and np.array_equal(n_docs[good], want[5]) and (stats[good, 3] == 0).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_a_call_is_one_search_and_one_late_interaction(name):
    index, orc, stored, dist = world(name)
    index.set_labels(search_labels())
    Q = MC.near_far_queries(stored, T3, NQ, QUERY_SEED)
    index.search_batch_late(Q, TOPN, POOL, EF)  # (the snapshot and the labels are in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q.reshape(NQ * T3, -1), POOL, EF)
    keys = ("late_calls", "late_launches", "uploads", "label_words_uploaded")
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_late(Q, TOPN, POOL, EF, mode="sum_sq")
    fk = kernel_of(index)
    assert log.get(fk) == 1 and fk not in plain, (dict(log), dict(plain))
    assert {k: v for k, v in log.items() if k != fk} == dict(plain), (dict(log), dict(plain))  # one search, as the plain call
    assert {k: index.stat(k) for k in keys} == {"late_calls": before["late_calls"] + 1, "late_launches": before["late_launches"] + 1,
                                                "uploads": before["uploads"],
                                                "label_words_uploaded": before["label_words_uploaded"]}


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_under_deletions(name):
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    Q = MC.near_far_queries(stored, T3, 32, 13)
    found = np.asarray(orc.search_batch(Q.reshape(32 * T3, -1), 8, EF)[0])
    deleted = np.unique(found[:, 1::3].reshape(-1))
    index.mark_deleted(deleted)
    try:
        pool = 64  # the limit while ids are deleted; T * pool = 192
        c = index.search_batch(Q.reshape(32 * T3, -1), pool, 64)
        want = H.late_interaction(Q, "sum", c[0].reshape(32, T3, pool), c[2].reshape(32, T3), c[3][:, 3].reshape(32, T3), dist,
                                  labels, TOPN, N)
        got = index.search_batch_late(Q, TOPN, pool, 64)
        LC.assert_late_equal(got[:6], want, name)
        assert np.array_equal(got[6], summed_stats(c[3].reshape(32, T3, 4), want[6])), "stats are the candidate call's, summed"
        assert (got[4] == TOPN).all() and not np.isin(got[2], deleted).any()
        with pytest.raises(H.HnswError) as e:
            index.search_batch_late(Q, TOPN, pool + 1, 64)
        assert e.value.code == _lib.ERR_ARG and "pool <= 64 while ids are deleted" in str(e.value)
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_late(Q, TOPN, 85, 128)  # nothing deleted: the unfiltered limits again
    assert (got[4] == TOPN).all()


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_cosine_option(kind):
    n, d = 1200, 24
    vs = (rand_vectors(n, d, 91) - np.float32(0.3)).astype(np.float32)
    lv = O.draw_levels(n, M, 9)
    index = H.HNSW.new(M, 32, d, kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=lv)
    labels = (np.arange(n) % 53).astype(np.uint32)
    index.set_labels(labels)
    # the oracle: a plain index over rows normalised beforehand by the option's arithmetic, asked with unit queries
    orc = oracle_from_product(index, SC.unit(vs), lv)
    dist = LC.memo(orc.distance_batch)
    Q = MC.near_far_queries(vs, T3, NQ, 17)
    Qu = SC.unit(Q.reshape(NQ * T3, d)).reshape(NQ, T3, d)
    c_ids, c_counts, c_stats = oracle_lists(orc, Qu, POOL, EF)
    for mode in ("sum", "sum_sq"):
        want = H.late_interaction(Qu, mode, c_ids, c_counts, None, dist, labels, TOPN, n)
        got = index.search_batch_late(Q, TOPN, POOL, EF, mode=mode)
        LC.assert_late_equal(got[:6], want, "cosine " + mode)
        assert np.array_equal(got[6], summed_stats(c_stats, want[6]))
    # the primitive makes its own unit copy of the caller's raw vectors
    got, log = late_on_device(index, Q, "sum_sq", c_ids, c_counts, c_stats, TOPN)
    LC.assert_late_equal(got[:6], H.late_interaction(Qu, "sum_sq", c_ids, c_counts, None, dist, labels, TOPN, n), "cosine primitive")
    assert log.get(kernel_of(index)) == 1


# ---- 4. capture and replay ------------------------------------------------------------------------------------------------
CAP_T, CAP_POOL = 3, 16
OUT_SHAPES = {"labels": (NQ, TOPN), "scores": (NQ, TOPN), "best": (NQ, TOPN), "sizes": (NQ, TOPN), "counts": (NQ,),
              "n_docs": (NQ,), "stats": (NQ, 4)}


def cap_lists(stored, seed):
    """NQ queries, every one legal (the replayed bytes are compared, statuses included)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, N, (NQ, CAP_T, CAP_POOL)).astype(np.uint32)
    counts = rng.integers(1, CAP_POOL + 1, (NQ, CAP_T)).astype(np.uint32)
    stats = rng.integers(0, 2 ** 31, (NQ, CAP_T, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    Q = stored[rng.integers(0, N, (NQ, CAP_T))] + rng.normal(0, 0.05, (NQ, CAP_T, stored.shape[1])).astype(np.float32)
    return np.ascontiguousarray(Q, dtype=np.float32), ids, counts, stats


def as_bits(w, stats):
    return w[0], w[1].view(np.uint32), w[2], w[3], w[4], w[5], summed_stats(stats, w[6]).astype(np.uint32)


@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_the_primitive_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name):
    import torch
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    index.upload()
    lists = {"real": cap_lists(stored, 31), "decoy": cap_lists(stored, 32)}
    names = ("Q", "ids_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}

    def enqueue(i, o, stream):
        index.late_interaction_device(NQ, CAP_T, CAP_POOL, TOPN, "sum", i["Q"], i["ids_in"], i["counts_in"], i["stats_in"],
                                      o["labels"], o["scores"], o["best"], o["sizes"], o["counts"], o["n_docs"], o["stats"], stream)

    def want(which):
        Q, ids, counts, stats = lists[which]
        w = H.late_interaction(Q, "sum", ids, counts, None, dist, labels, TOPN, N)
        assert (w[6] == 0).all()
        return as_bits(w, stats)

    call = SC.Call(torch, "late", inputs, OUT_SHAPES, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {kernel_of(index): 1})  # (its direct calls bring the label column to HBM)


@pytest.mark.parametrize("name", ["f32-100", "quant8-100"])
def test_the_chain_search_late_is_two_nodes_and_replays_the_direct_calls_bytes(name):
    """inside the capture conditions of hnsw_search_batch_device (ef <= 256, nothing deleted, cosine off); both launches
    are enqueued on ONE stream, so the captured graph is one chain without parallel branches.  _finish synchronises and is
    no part of a captured graph: the direct chain is run with it as well, to the same bytes."""
    import torch
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    index.upload()
    qs = {"real": MC.near_far_queries(stored, T3, NQ, 41), "decoy": MC.near_far_queries(stored, T3, NQ, 42)}
    inputs = {"Q": (qs["real"], qs["decoy"])}
    dev = torch.device("cuda:0")
    rows = NQ * T3
    mid = {"ids": torch.zeros((rows, POOL), dtype=torch.int32, device=dev),
           "dists": torch.zeros((rows, POOL), dtype=torch.int32, device=dev),
           "counts": torch.zeros(rows, dtype=torch.int32, device=dev),
           "stats": torch.zeros((rows, 4), dtype=torch.int32, device=dev)}

    def search_args(i, stream):
        return (i["Q"].data_ptr(), rows, POOL, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(), mid["counts"].data_ptr(),
                mid["stats"].data_ptr(), stream)

    def enqueue(i, o, stream, finish=False):
        index.search_batch_device(*search_args(i, stream))
        if finish:
            index.search_batch_device_finish(*search_args(i, stream))
        index.late_interaction_device(NQ, T3, POOL, TOPN, "sum_sq", i["Q"], mid["ids"], mid["counts"], mid["stats"], o["labels"],
                                      o["scores"], o["best"], o["sizes"], o["counts"], o["n_docs"], o["stats"], stream)

    def want(which):
        c_ids, c_counts, c_stats = oracle_lists(orc, qs[which], POOL, EF)
        w = H.late_interaction(qs[which], "sum_sq", c_ids, c_counts, None, dist, labels, TOPN, N)
        return as_bits(w, c_stats)

    call = SC.Call(torch, "chain", inputs, OUT_SHAPES, enqueue)
    call.want = want
    call.distinguishable()
    # the direct chain with _finish in it
    call.load("real")
    call.poison()
    enqueue(call.inp, call.out, torch.cuda.current_stream().cuda_stream, finish=True)
    torch.cuda.synchronize()
    assert SC.verdict(call.arrays(copies=False), want("real")) is None
    with H.kernel_log() as plain:
        index.search_batch_device(*search_args(call.inp, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert sum(plain.values()) == 1, dict(plain)
    expected = dict(plain)
    expected[kernel_of(index)] = 1
    capture_and_replay(torch, call, want, expected)
