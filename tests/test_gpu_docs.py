"""Exact document scoring on the GPU (include/hnsw_mi355x.h, "exact document scoring"), held to the numpy restatement
(hnsw_rs_amd.docs.score_documents; tests/test_docs_host.py holds that to a plain loop) over the CPU oracle's distances
(OracleHNSW.distance_batch) and search (OracleHNSW.search_batch).  All comparisons are exact: labels, score BITS, best ids,
sizes, counts, n_docs, counters and statuses.
  1. hnsw_score_documents_device alone: one launch and nothing else, guard words, no word unwritten; label columns whose
     scored rows total the pass boundaries of both vector kinds and the chunk's end, a document that straddles the chunk
     boundary, one larger than a chunk, documents at rows_cap, 256 documents, T = 1, 3, 32, both modes;
  2. handle states: no labels, ids inserted behind the column, deletions inside a document and of a whole one,
     relabelling, and the document index's upload counter through all of it;
  3. a planted meaning: the query made of a document's own rows finds that document first with score +0;
  4. search_batch_late_exact against the restatements chained over the ORACLE's lists; deletions, the cosine option,
     launch accounting; and the property the feature exists for: every returned score is the exhaustive one;
  5. capture and replay of the primitive and of the chain search -> late interaction -> scoring on a torch stream.
The indexes are built by the recipe of tests/test_gpu_from_rows.py in a cache of this file's own: these tests set labels,
and the shared ones stay unchanged.  Every test sets the label column it needs."""
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import docs_cases as DC
from tests import multi_cases as MC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import M, N, SHAPES, capture_and_replay, guarded, kernel_of, unguard, up
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
NQ = 6
NOBODY = 777777  # a label no column here has
DOC_KEYS = ("doc_index_uploads", "doc_index_keys_uploaded")


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
    return index, orc, stored, DC.memo(orc.distance_batch)


def vectors(stored, nq, T, seed):
    rng = np.random.default_rng(seed)
    Q = stored[rng.integers(0, stored.shape[0], (nq, T))] + rng.normal(0, 0.05, (nq, T, stored.shape[1])).astype(np.float32)
    return np.ascontiguousarray(Q, dtype=np.float32)


def lists_of(docs, n_in, nq, seed):
    """nq lists of n_in labels that name every label of `docs`, some twice, and NOBODY where room is left"""
    rng = np.random.default_rng(seed)
    docs = np.asarray(docs, dtype=np.uint32)
    assert docs.size <= n_in
    out = np.empty((nq, n_in), dtype=np.uint32)
    for q in range(nq):
        fill = rng.choice(np.concatenate([docs, [NOBODY]]).astype(np.uint32), n_in - docs.size)
        out[q] = rng.permutation(np.concatenate([docs, fill]))
    return out


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def docs_on_device(index, Q, mode, docs_in, counts, stats, n_out, rows_cap, extras=True):
    import torch
    nq, T = Q.shape[:2]
    n_in = docs_in.shape[1]
    d_in = (up(Q), up(docs_in), None if counts is None else up(counts), None if stats is None else up(stats.astype(np.uint32)))
    sizes = {"labels": nq * n_out, "scores": nq * n_out, "best": nq * n_out if extras else 0, "sizes": nq * n_out if extras else 0,
             "counts": nq if extras else 0, "n_docs": nq if extras else 0, "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.score_documents_device(nq, T, n_in, n_out, rows_cap, mode, d_in[0], d_in[1], d_in[2], d_in[3], out["labels"],
                                     out["scores"], out["best"], out["sizes"], out["counts"], out["n_docs"], out["stats"],
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shape = (nq, n_out)
    r = lambda k: None if got[k] is None else got[k].reshape(shape)  # noqa: E731
    return (r("labels"), got["scores"].view(np.float32).reshape(shape), r("best"), r("sizes"), got["counts"], got["n_docs"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4).astype(np.int64)), log


def held(index, dist, Q, mode, docs_in, counts, stats, labels, deleted, n_out, rows_cap, what, n_points=N):
    """the primitive against the restatement, one launch -> the restatement's answer"""
    statuses = None if stats is None else stats[:, 3].astype(np.uint32).view(np.int32).astype(np.int64)
    want = H.score_documents(Q, mode, docs_in, counts, statuses, dist, labels, deleted, n_out, rows_cap, n_points)
    got, log = docs_on_device(index, Q, mode, docs_in, counts, stats, n_out, rows_cap)
    assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
    DC.assert_late_equal(got[:6], want, what)
    if stats is not None:  # the incoming record, the status as decided
        exp = stats.astype(np.int64).copy()
        exp[:, 3] = want[6] & 0xFFFFFFFF
        assert np.array_equal(got[6], exp), what
    return want


def split(total):
    """a few document sizes that add up to `total`"""
    a = total // 3
    return [s for s in (a, a, total - 2 * a) if s > 0]


# the scored rows of a query: the pass boundaries of both vector kinds (32 and 64 entries a pass) and the chunk's end
TOTALS = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_primitive_alone_is_the_restatement_bit_for_bit(name, total):
    index, orc, stored, dist = world(name)
    sizes = split(total)
    labels = DC.column_of_sizes(N, sizes, first_label=5, rest=0)
    index.set_labels(labels)
    index.upload()
    T, n_in = 3, 8
    Q = vectors(stored, NQ, T, 100 * total + len(name))
    docs_in = lists_of(5 + np.arange(len(sizes)), n_in, NQ, total)
    counts = np.full(NQ, n_in, dtype=np.uint32)
    counts[1] = n_in + 9  # (above n_in: every entry)
    counts[2] = 0
    stats = np.random.default_rng(total).integers(2 ** 31, 2 ** 32, (NQ, 4)).astype(np.int64)
    stats[:, 3] = 0
    stats[3, 3] = _lib.ERR_OVERFLOW & 0xFFFFFFFF
    Q[4, T - 1, stored.shape[1] // 2] = np.nan
    launches = index.stat("docs_launches")
    for mode, n_out in ((H.LATE_SUM, 1), (H.LATE_SUM_SQ, n_in)):
        what = "%s total=%d mode=%d" % (name, total, mode)
        want = held(index, dist, Q, mode, docs_in, counts, stats, labels, None, n_out, 4096, what)
        assert want[6].tolist() == [0, 0, 0, _lib.ERR_OVERFLOW, _lib.ERR_NAN_INPUT, 0]
        assert want[5].tolist() == [len(sizes), len(sizes), 0, 0, 0, len(sizes)]  # NOBODY and duplicates are no documents
        if n_out == n_in:  # the scored rows of a query total `total`
            assert sorted(want[3][0, :want[4][0]].tolist()) == sorted(sizes) and want[3][5, :want[4][5]].sum() == total
    # bare: no counts (every entry present), no stats, no optional output
    got, log = docs_on_device(index, Q, H.LATE_SUM, docs_in, None, None, n_in, 4096, extras=False)
    want = H.score_documents(Q, H.LATE_SUM, docs_in, None, None, dist, labels, None, n_in, 4096, N)
    DC.assert_late_equal((got[0], got[1]), want, name + " bare")
    assert all(g is None for g in got[2:]) and dict(log) == {kernel_of(index): 1}
    assert want[5][2] == len(sizes) and want[5][3] == len(sizes)  # (without counts and statuses those lists are whole)
    assert index.stat("docs_launches") == launches + 3 and index.stat("docs_calls") == 0


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_documents_across_the_chunk_boundary_and_at_rows_cap(name):
    index, orc, stored, dist = world(name)
    Q = vectors(stored, NQ, 3, 77)
    # a document that straddles the chunk boundary: rows 1000 .. 1047 of the walk
    labels = DC.column_of_sizes(N, [1000, 48, 20], first_label=1, rest=MAX)
    index.set_labels(labels)
    docs_in = np.tile(np.array([1, 2, 3, MAX], dtype=np.uint32), (NQ, 1))
    want = held(index, dist, Q, "sum", docs_in, None, None, labels, None, 4, 4096, name + " straddle")
    assert sorted(want[3][0].tolist()) == [20, 48, 432, 1000] and (want[4] == 4).all()
    # one document larger than a chunk, whole and then cut by one
    labels = DC.column_of_sizes(N, [1100], first_label=MAX, rest=0)
    index.set_labels(labels)
    docs_in = np.tile(np.array([MAX, 0], dtype=np.uint32), (NQ, 1))
    whole = held(index, dist, Q, "sum_sq", docs_in, None, None, labels, None, 2, 1100, name + " 1100")
    cut = held(index, dist, Q, "sum_sq", docs_in, None, None, labels, None, 2, 1099, name + " 1099")
    for w in (whole, cut):
        assert sorted(w[3][0].tolist()) == [400, 1100] and (w[5] == 2).all()
    # document sizes 1 and rows_cap - 1, rows_cap, rows_cap + 1 at rows_cap = 64
    labels = DC.column_of_sizes(N, [1, 63, 64, 65], first_label=10, rest=0)
    index.set_labels(labels)
    docs_in = lists_of([10, 11, 12, 13], 6, NQ, 3)
    want = held(index, dist, Q, "sum", docs_in, None, None, labels, None, 4, 64, name + " rows_cap")
    assert sorted(want[3][0].tolist()) == [1, 63, 64, 65]
    assert (want[2] < 1 + 63 + 64 + 64).all()  # (id 192, the 65th row of document 13, is never scored)


@pytest.mark.parametrize("T", [1, 3, 32])
@pytest.mark.parametrize("n_in", [1, 64, 65, 256])
@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_many_documents_of_one_row_each(name, n_in, T):
    index, orc, stored, dist = world(name)
    labels = (1000 + np.arange(N)).astype(np.uint32)
    labels[256:] = 0
    index.set_labels(labels)
    Q = vectors(stored, 4, T, n_in + T)
    rng = np.random.default_rng(n_in)
    docs_in = np.stack([rng.permutation(256)[:n_in] + 1000 for _ in range(4)]).astype(np.uint32)
    for mode in ("sum", "sum_sq"):
        want = held(index, dist, Q, mode, docs_in, None, None, labels, None, min(10, n_in), 5, "%s n_in=%d T=%d" % (name, n_in, T))
        assert (want[5] == n_in).all() and (want[3][:, 0] == 1).all() and (want[2][:, 0] + 1000 == want[0][:, 0]).all()


# ---- 2. handle states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_no_labels_then_a_column_then_ids_inserted_behind_it(kind):
    n0, n1, d = 500, 600, 20
    vs = rand_vectors(n1, d, 17)
    lv = O.draw_levels(n1, M, 5)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(vs[:n0], 4, False, levels=lv[:n0])
    orc = oracle_from_product(index, vs[:n0], lv[:n0])
    Q = vectors(vs, 4, 3, 9)
    docs_in = np.tile(np.array([0, 3, NOBODY], dtype=np.uint32), (4, 1))
    # an unlabelled handle: label 0 is the whole index, cut at rows_cap
    want = held(index, orc.distance_batch, Q, "sum", docs_in, None, None, None, None, 2, 100, "no labels", n0)
    assert (want[5] == 1).all() and (want[0][:, 0] == 0).all() and (want[3][:, 0] == n0).all() and (want[2][:, 0] < 100).all()
    assert index.stat("doc_index_uploads") == 1 and index.stat("doc_index_keys_uploaded") == n0
    column = (1 + np.arange(n0) % 7).astype(np.uint32)
    index.set_labels(column)
    want = held(index, orc.distance_batch, Q, "sum", docs_in, None, None, column, None, 2, 100, "a column", n0)
    assert (want[5] == 1).all() and (want[0][:, 0] == 3).all()  # no id has label 0 now
    assert index.stat("doc_index_uploads") == 2
    # ids inserted after the column was set: label 0, beyond the column
    index.insert_bulk(vs[n0:], 4, False, levels=lv[n0:])
    orc = oracle_from_product(index, vs, lv)
    want = held(index, orc.distance_batch, Q, "sum_sq", docs_in, None, None, column, None, 2, 100, "inserted", n1)
    assert (want[5] == 2).all() and sorted(want[3][0].tolist()) == sorted([n1 - n0, int((column == 3).sum())])
    assert index.stat("doc_index_uploads") == 3 and index.stat("doc_index_keys_uploaded") == n0 + n0 + n1


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_deletions_relabelling_and_the_index_uploads(name):
    index, orc, stored, dist = world(name)
    labels = (np.arange(N) % 50).astype(np.uint32)  # 50 documents of 30 rows
    index.set_labels(labels)
    Q = vectors(stored, NQ, 3, 21)
    docs_in = lists_of([4, 5, 6, 7], 6, NQ, 5)
    held(index, dist, Q, "sum", docs_in, None, None, labels, None, 4, 4096, name)
    ups = index.stat("doc_index_uploads")
    held(index, dist, Q, "sum_sq", docs_in, None, None, labels, None, 4, 4096, name)
    assert index.stat("doc_index_uploads") == ups  # nothing changed: nothing moves
    inside = np.array([4, 54, 1454, 5], dtype=np.uint32)  # three rows of document 4 (its lowest ids among them), one of 5
    whole = np.flatnonzero(labels == 6).astype(np.uint32)  # document 6 entirely
    dead = np.concatenate([inside, whole])
    index.mark_deleted(dead)
    try:
        want = held(index, dist, Q, "sum", docs_in, None, None, labels, dead, 4, 4096, name + " deleted")
        assert (want[5] == 3).all() and not np.isin(want[0], 6).any() and not np.isin(want[2], dead).any()
        assert sorted(want[3][0, :3].tolist()) == [27, 29, 30]
        assert index.stat("doc_index_uploads") == ups + 1
        held(index, dist, Q, "sum", docs_in, None, None, labels, dead, 4, 2, name + " deleted, cut")  # the lowest LIVE ids
        assert index.stat("doc_index_uploads") == ups + 1
    finally:
        index.unmark_deleted(dead)
    want = held(index, dist, Q, "sum", docs_in, None, None, labels, None, 4, 4096, name + " unmarked")
    assert (want[5] == 4).all() and index.stat("doc_index_uploads") == ups + 2
    relabelled = labels.copy()
    relabelled[labels == 7] = 4  # document 7 joins document 4
    index.set_labels(relabelled)
    want = held(index, dist, Q, "sum", docs_in, None, None, relabelled, None, 4, 4096, name + " relabelled")
    assert (want[5] == 3).all() and 60 in want[3][0].tolist() and index.stat("doc_index_uploads") == ups + 3
    held(index, dist, Q, "sum", docs_in, None, None, relabelled, None, 4, 4096, name + " again")
    assert index.stat("doc_index_uploads") == ups + 3


# ---- 3. a planted meaning ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-16", "f32-100"])
def test_the_query_made_of_a_documents_rows_finds_it_first_with_score_zero(name):
    index, orc, stored, dist = world(name)
    labels = (np.arange(N) // 4).astype(np.uint32)  # documents of 4 consecutive ids
    index.set_labels(labels)
    rng = np.random.default_rng(9)
    docs = rng.choice(np.arange(30, 340), 8, replace=False)  # (clear of the twin rows)
    Q = np.ascontiguousarray(np.stack([stored[4 * x:4 * x + 4] for x in docs]), dtype=np.float32)
    docs_in = rng.integers(0, N // 4, (8, 12)).astype(np.uint32)
    docs_in[np.arange(8), rng.integers(0, 12, 8)] = docs
    for mode in ("sum", "sum_sq"):
        want = held(index, dist, Q, mode, docs_in, None, None, labels, None, 5, 4096, name + " " + mode)
        assert (want[0][:, 0] == docs).all() and (want[1][:, 0].view(np.uint32) == 0).all()  # score +0
        assert (want[3][:, 0] == 4).all() and (want[2][:, 0] == 4 * docs).all()  # its full size; the smallest id of them
        assert (want[1][:, 1] > 0).all() and (want[4] == 5).all()


# ---- 4. the search against the chained restatements of the oracle's lists -------------------------------------------------
T3, POOL, TOPN, NCAND, EF = 3, 16, 10, 24, 32
SNQ = 32


def oracle_lists(orc, Q, pool, ef):
    nq, T = Q.shape[:2]
    c = orc.search_batch(Q.reshape(nq * T, -1), pool, ef)
    stats = np.concatenate([np.asarray(c[3]).astype(np.int64), np.zeros((nq * T, 1), dtype=np.int64)], axis=1)
    return np.asarray(c[0]).reshape(nq, T, pool), np.asarray(c[2]).reshape(nq, T), stats.reshape(nq, T, 4)


def chained(Q, mode, c_ids, c_counts, c_statuses, dist, labels, deleted, n, n_cand, rows_cap, n_points=N):
    """THE DOCUMENT SCORING of the labels, counts and statuses THE LATE INTERACTION returns -> (the scoring, the late interaction)"""
    late = H.late_interaction(Q, mode, c_ids, c_counts, c_statuses, dist, labels, n_cand, n_points)
    return H.score_documents(Q, mode, late[0], late[4], late[6], dist, labels, deleted, n, rows_cap, n_points), late


def summed(c_stats, statuses):
    s = (np.asarray(c_stats).astype(np.uint64)[:, :, :3].sum(axis=1) & 0xFFFFFFFF).astype(np.int64)
    return np.concatenate([s, (np.asarray(statuses).astype(np.int64) & 0xFFFFFFFF)[:, None]], axis=1)


def search_labels():
    return (np.arange(N) % 61).astype(np.uint32)  # 61 documents of 24 or 25 rows spread over the index


@pytest.mark.parametrize("name", list(SHAPES))
def test_search_is_the_scoring_of_the_late_interaction_of_the_oracles_lists(name):
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    for T in (T3, 1):
        Q = MC.near_far_queries(stored, T, SNQ, 7)
        c_ids, c_counts, c_stats = oracle_lists(orc, Q, POOL, EF)
        n_cand = min(NCAND, T * POOL)
        for mode, rows_cap in (("sum", H.DOCS_MAX_ROWS), ("sum_sq", 9)):
            what = "%s T=%d mode=%s" % (name, T, mode)
            want, late = chained(Q, mode, c_ids, c_counts, None, dist, labels, None, TOPN, n_cand, rows_cap)
            got = index.search_batch_late_exact(Q, TOPN, n_cand, POOL, EF, mode=mode, rows_cap=rows_cap)
            DC.assert_late_equal(got[:6], want, what)
            assert np.array_equal(got[6], summed(c_stats, want[6])), what
            taken = np.arange(TOPN)[None, :] < got[4][:, None]
            assert (got[5] == late[4]).all() and (got[4] == np.minimum(got[5], TOPN)).all() and (got[3][taken] >= 24).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_every_returned_score_is_the_exhaustive_one_where_the_pools_fall_short(name):
    """the property the feature exists for, on the planted index: documents of 25 rows, pools of 16 -- the late
    interaction cannot have seen every row of a document, the exact call scores them all"""
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    Q = MC.near_far_queries(stored, T3, SNQ, 19)
    c_ids, c_counts, c_stats = oracle_lists(orc, Q, POOL, EF)
    want, late = chained(Q, "sum", c_ids, c_counts, None, dist, labels, None, TOPN, NCAND, H.DOCS_MAX_ROWS)
    approx = H.late_interaction(Q, "sum", c_ids, c_counts, None, dist, labels, TOPN, N)

    def exhaustive(q, g):
        rows = np.flatnonzero(labels == g).astype(np.uint32)
        s = None
        for t in range(T3):
            m = np.float32(np.min(dist(Q[q, t], rows)))
            s = m if s is None else np.float32(s + m)
        return s

    # asked of the restatements first: the shortcut's scores differ from the exhaustive ones, the chained ones do not
    differs = 0
    for q in range(SNQ):
        for k in range(int(approx[4][q])):
            differs += approx[1][q, k].view(np.uint32) != exhaustive(q, int(approx[0][q, k])).view(np.uint32)
    assert differs > 0, "the pools cover every document: the test would pass vacuously"
    got = index.search_batch_late_exact(Q, TOPN, NCAND, POOL, EF)
    late_got = index.search_batch_late(Q, TOPN, POOL, EF)
    DC.assert_late_equal(late_got[:6], approx, name + " late")
    DC.assert_late_equal(got[:6], want, name)
    n_diff = 0
    for q in range(SNQ):
        assert got[4][q] == min(TOPN, int(late[4][q])) and got[4][q] > 0
        for k in range(int(got[4][q])):
            assert got[1][q, k].view(np.uint32) == exhaustive(q, int(got[0][q, k])).view(np.uint32), (q, k)
        for k in range(int(late_got[4][q])):
            n_diff += late_got[1][q, k].view(np.uint32) != exhaustive(q, int(late_got[0][q, k])).view(np.uint32)
    assert n_diff == differs and n_diff > 0


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_under_deletions(name):
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    Q = MC.near_far_queries(stored, T3, SNQ, 13)
    found = np.asarray(orc.search_batch(Q.reshape(SNQ * T3, -1), 8, EF)[0])
    deleted = np.unique(found[:, 1::3].reshape(-1))
    index.mark_deleted(deleted)
    try:
        pool = 64  # the limit while ids are deleted; T * pool = 192
        c = index.search_batch(Q.reshape(SNQ * T3, -1), pool, 64)
        want, late = chained(Q, "sum", c[0].reshape(SNQ, T3, pool), c[2].reshape(SNQ, T3), c[3][:, 3].reshape(SNQ, T3), dist,
                             labels, deleted, TOPN, 32, H.DOCS_MAX_ROWS)
        got = index.search_batch_late_exact(Q, TOPN, 32, pool, 64)
        DC.assert_late_equal(got[:6], want, name)
        assert np.array_equal(got[6], summed(c[3].reshape(SNQ, T3, 4), want[6])), "stats are the candidate call's, summed"
        assert (got[4] == TOPN).all() and not np.isin(got[2], deleted).any()
        live = np.bincount(labels[np.setdiff1d(np.arange(N), deleted)], minlength=61)
        assert (got[3] == live[got[0]]).all()  # the sizes count the undeleted rows
        with pytest.raises(H.HnswError) as e:
            index.search_batch_late_exact(Q, TOPN, 32, pool + 1, 64)
        assert e.value.code == _lib.ERR_ARG and "pool <= 64 while ids are deleted" in str(e.value)
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_late_exact(Q, TOPN, 32, 85, 128)  # nothing deleted: the unfiltered limits again
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
    dist = DC.memo(orc.distance_batch)
    Q = MC.near_far_queries(vs, T3, SNQ, 17)
    Qu = SC.unit(Q.reshape(SNQ * T3, d)).reshape(SNQ, T3, d)
    c_ids, c_counts, c_stats = oracle_lists(orc, Qu, POOL, EF)
    for mode in ("sum", "sum_sq"):
        want, late = chained(Qu, mode, c_ids, c_counts, None, dist, labels, None, TOPN, NCAND, H.DOCS_MAX_ROWS, n)
        got = index.search_batch_late_exact(Q, TOPN, NCAND, POOL, EF, mode=mode)
        DC.assert_late_equal(got[:6], want, "cosine " + mode)
        assert np.array_equal(got[6], summed(c_stats, want[6]))
    # the primitive makes its own unit copy of the caller's raw vectors
    docs_in = np.tile(np.arange(12, dtype=np.uint32), (SNQ, 1))
    got, log = docs_on_device(index, Q, "sum_sq", docs_in, None, None, 12, 4096)
    DC.assert_late_equal(got[:6], H.score_documents(Qu, "sum_sq", docs_in, None, None, dist, labels, None, 12, 4096, n), "cosine primitive")
    assert log.get(kernel_of(index)) == 1


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_a_call_is_one_search_one_late_interaction_and_one_scoring(name):
    index, orc, stored, dist = world(name)
    index.set_labels(search_labels())
    Q = MC.near_far_queries(stored, T3, SNQ, 7)
    index.search_batch_late_exact(Q, TOPN, NCAND, POOL, EF)  # (the snapshot, the labels and the document index are in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q.reshape(SNQ * T3, -1), POOL, EF)
    keys = ("docs_calls", "docs_launches", "late_calls", "late_launches", "uploads", "label_words_uploaded") + DOC_KEYS
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_late_exact(Q, TOPN, NCAND, POOL, EF, mode="sum_sq")
    fk = kernel_of(index)
    assert log.get(fk) == 2 and fk not in plain, (dict(log), dict(plain))  # the late interaction and the scoring
    assert {k: v for k, v in log.items() if k != fk} == dict(plain), (dict(log), dict(plain))  # one search, as the plain call
    after = dict(before)
    after["docs_calls"] += 1
    after["docs_launches"] += 1
    after["late_launches"] += 1
    assert {k: index.stat(k) for k in keys} == after


# ---- 5. capture and replay ------------------------------------------------------------------------------------------------
CNQ = 64
OUT_SHAPES = {"labels": (CNQ, TOPN), "scores": (CNQ, TOPN), "best": (CNQ, TOPN), "sizes": (CNQ, TOPN), "counts": (CNQ,),
              "n_docs": (CNQ,), "stats": (CNQ, 4)}


def as_bits(w, stats4):
    return w[0], w[1].view(np.uint32), w[2], w[3], w[4], w[5], stats4.astype(np.uint32)


def cap_lists(stored, seed):
    """CNQ lists of 20 labels of search_labels' documents, every one legal (the replayed bytes are compared, statuses included)"""
    rng = np.random.default_rng(seed)
    docs_in = rng.integers(0, 61, (CNQ, 20)).astype(np.uint32)
    counts = rng.integers(1, 21, CNQ).astype(np.uint32)
    stats = rng.integers(0, 2 ** 31, (CNQ, 4)).astype(np.int64)
    stats[:, 3] = 0
    return vectors(stored, CNQ, T3, seed), docs_in, counts, stats


@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_the_primitive_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name):
    import torch
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    index.upload()
    lists = {"real": cap_lists(stored, 31), "decoy": cap_lists(stored, 32)}
    names = ("Q", "docs_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}

    def enqueue(i, o, stream):
        index.score_documents_device(CNQ, T3, 20, TOPN, 12, "sum", i["Q"], i["docs_in"], i["counts_in"], i["stats_in"],
                                     o["labels"], o["scores"], o["best"], o["sizes"], o["counts"], o["n_docs"], o["stats"], stream)

    def want(which):
        Q, docs_in, counts, stats = lists[which]
        w = H.score_documents(Q, "sum", docs_in, counts, None, dist, labels, None, TOPN, 12, N)
        assert (w[6] == 0).all()
        return as_bits(w, stats)

    call = SC.Call(torch, "docs", inputs, OUT_SHAPES, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {kernel_of(index): 1})  # (its direct calls bring the document index to HBM)


@pytest.mark.parametrize("name", ["f32-100", "quant8-100"])
def test_the_chain_search_late_scoring_is_three_nodes_and_replays_the_direct_calls_bytes(name):
    """inside the capture conditions of hnsw_search_batch_device (ef <= 256, nothing deleted, cosine off); the three
    launches are enqueued on ONE stream, so the captured graph is one chain without parallel branches"""
    import torch
    index, orc, stored, dist = world(name)
    labels = search_labels()
    index.set_labels(labels)
    index.upload()
    qs = {"real": MC.near_far_queries(stored, T3, CNQ, 41), "decoy": MC.near_far_queries(stored, T3, CNQ, 42)}
    inputs = {"Q": (qs["real"], qs["decoy"])}
    dev = torch.device("cuda:0")
    rows = CNQ * T3
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    mid = {"ids": z(rows, POOL), "dists": z(rows, POOL), "counts": z(rows), "stats": z(rows, 4)}
    doc = {"labels": z(CNQ, NCAND), "scores": z(CNQ, NCAND), "counts": z(CNQ), "stats": z(CNQ, 4)}

    def search_args(i, stream):
        return (i["Q"].data_ptr(), rows, POOL, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(), mid["counts"].data_ptr(),
                mid["stats"].data_ptr(), stream)

    def enqueue(i, o, stream):
        index.search_batch_device(*search_args(i, stream))
        index.late_interaction_device(CNQ, T3, POOL, NCAND, "sum_sq", i["Q"], mid["ids"], mid["counts"], mid["stats"], doc["labels"],
                                      doc["scores"], None, None, doc["counts"], None, doc["stats"], stream)
        index.score_documents_device(CNQ, T3, NCAND, TOPN, H.DOCS_MAX_ROWS, "sum_sq", i["Q"], doc["labels"], doc["counts"],
                                     doc["stats"], o["labels"], o["scores"], o["best"], o["sizes"], o["counts"], o["n_docs"],
                                     o["stats"], stream)

    def want(which):
        c_ids, c_counts, c_stats = oracle_lists(orc, qs[which], POOL, EF)
        w, late = chained(qs[which], "sum_sq", c_ids, c_counts, None, dist, labels, None, TOPN, NCAND, H.DOCS_MAX_ROWS)
        return as_bits(w, summed(c_stats, w[6]))

    call = SC.Call(torch, "chain", inputs, OUT_SHAPES, enqueue)
    call.want = want
    call.distinguishable()
    with H.kernel_log() as plain:
        index.search_batch_device(*search_args({"Q": up(qs["real"])}, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert sum(plain.values()) == 1, dict(plain)
    expected = dict(plain)
    expected[kernel_of(index)] = 2
    capture_and_replay(torch, call, want, expected)
