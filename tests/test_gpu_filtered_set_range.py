"""A label range AND a row of a resident mask set in one filtered search on the MI355X:
hnsw_search_batch_filtered_set_range against hnsw_search_batch_filtered_multi with the conjunctions materialised as
masks (ids, distance bits, counts, stats, paths) and against the CPU restatement (tests/filtered_restate.py) under the
predicate itself; every compiled form of the graph kernel; the compaction at its edges; what stays in HBM and in the
set's caches between calls; the device-pointer form against the host form with filter_exact_max = -1."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import LIMIT, restated
from tests.test_gpu_filtered_multi import (FORMS, NONE, check_rows, compare_row, glove, graph_kernels,  # noqa: F401
                                           predicates, raw_multi)
from tests.test_gpu_mask_set import delta, same, stats_of, three_paths  # noqa: F401
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
STATS = ("filtered_set_range_calls", "filtered_set_range_groups", "label_words_uploaded", "mask_set_words_uploaded",
         "mask_set_recounts", "mask_set_compactions", "uploads", "filtered_set_calls", "filtered_range_calls")
PATH_STATS = ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact")


def as_multi(n_points, rows_b, labels, mo, lo, hi):
    """the (row, lo, hi) triples of a call as the masks and mask_of of the equivalent _multi call: one mask over the
    index per distinct triple, `row AND lo <= label <= hi` (a row's bits at and beyond its length do not count, a label
    that was never set is 0); (HNSW_MASK_NONE, [0, UINT32_MAX]) stays HNSW_MASK_NONE"""
    lab = np.zeros(n_points, dtype=np.int64)
    k = min(n_points, len(labels))
    lab[:k] = np.asarray(labels, dtype=np.int64)[:k]
    mask_list, where, out = [], {}, []
    for g, l, h in zip(mo, lo, hi):
        key = (int(g), int(l), int(h))
        if key == (NONE, 0, MAX):
            out.append(NONE)
            continue
        if key not in where:
            m = (lab >= key[1]) & (lab <= key[2])
            if key[0] != NONE:
                row = np.zeros(n_points, dtype=bool)
                r = np.asarray(rows_b[key[0]], dtype=bool)
                kk = min(n_points, r.shape[0])
                row[:kk] = r[:kk]
                m &= row
            where[key] = len(mask_list)
            mask_list.append(m)
        out.append(where[key])
    return mask_list, np.array(out)


def both_and_multi(index, s, Q, n, ef, rows_b, labels, mo, lo, hi, exact_max, what=""):
    """the combined call and the _multi call with the conjunctions as masks: equal -> the combined call's result and
    the conjunction masks"""
    index.set_option("filter_exact_max", exact_max)
    got = index.search_batch_filtered_set_range(Q, n, ef, s, mo, lo, hi)
    mask_list, cmo = as_multi(index.len(), rows_b, labels, mo, lo, hi)
    same(got, index.search_batch_filtered_multi(Q, n, ef, mask_list, cmo), what)
    return got, mask_list, cmo


def raw_both(index, s, Q, n, ef, mo, lo, hi):
    """the C entry itself -> status and the five arrays (the Python mirror raises on a per-query error)"""
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    mo = np.where(np.asarray(mo) < 0, H.MASK_NONE, mo).astype(np.uint32)
    lo, hi = np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)
    ids = np.full((nq, n), _lib.UINT32_MAX, dtype=np.uint32)
    dists = np.full((nq, n), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    stats = np.zeros((nq, 4), dtype=np.int32)
    paths = np.zeros(nq, dtype=np.uint8)

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    rc = _lib.lib().hnsw_search_batch_filtered_set_range(
        index._h, p(Q, C.c_float), nq, n, ef, s._s, p(mo, C.c_uint32), p(lo, C.c_uint32), p(hi, C.c_uint32),
        p(ids, C.c_uint32), p(dists, C.c_float), p(counts, C.c_uint32), C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)),
        p(paths, C.c_uint8))
    return rc, (ids, dists, counts, stats.astype(np.int64), paths)


def device_call(index, s, Q, n, ef, mo, lo, hi, optional=True, log_enqueue=None):
    """the device form with torch tensors in HBM, completed by _finish -> (status or None, the five arrays)"""
    import torch
    dev = torch.device("cuda:0")
    nq = Q.shape[0]

    def u32(a):
        return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    dQ = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    d_mo = None if mo is None else u32(np.where(np.asarray(mo) < 0, H.MASK_NONE, mo))
    d_lo, d_hi = u32(lo), u32(hi)
    d_ids = torch.zeros((nq, n), dtype=torch.int32, device=dev)
    d_d = torch.zeros((nq, n), dtype=torch.float32, device=dev)
    d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_s = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    args = (dQ, nq, n, ef, s, d_mo, d_lo, d_hi, d_ids, d_d if optional else None, d_c if optional else None, d_s, 0)
    torch.cuda.synchronize(dev)
    if log_enqueue is not None:
        with H.kernel_log() as log:
            index.search_batch_filtered_set_range_device(*args)
        log_enqueue.update(log)
    else:
        index.search_batch_filtered_set_range_device(*args)
    code = None
    paths = np.zeros(nq, dtype=np.uint8)
    try:
        paths = index.search_batch_filtered_set_range_device_finish(*args, paths=True)
    except H.HnswError as e:
        code = e.code
    torch.cuda.synchronize(dev)
    return code, (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                  d_s.cpu().numpy().view(np.uint32).astype(np.int64), paths)


# ---- 1. all three paths in one call, f32 and 8-bit; the same under deletions ----------------------------------------
def three_path_halves(mask_list):
    """labels and rows over the fixture's 30000 ids such that neither half of a conjunction decides the path alone:
    row 0 AND [3, 3] is exactly `sparse` (16 ids), row 1 AND [5, 5] exactly the six ids, row 2 AND [1, 3] thousands --
    while every row and every one of those ranges allows thousands of ids on its own"""
    dense, sparse, six = mask_list
    n = 30000
    rng = np.random.default_rng(85)
    u, v = rng.random(n), rng.random(n)
    lab = np.where(u < 0.25, 3, np.where(u < 0.5, 5, 1)).astype(np.uint32)
    rows = np.zeros((3, n), dtype=bool)
    rows[0] = (lab != 3) & (v < 0.5)  # thousands of ids, none of them labelled 3 ...
    rows[1] = (lab != 5) & (v >= 0.5)
    rows[2] = dense
    six_b = np.zeros(n, dtype=bool)
    six_b[six] = True
    assert not (six_b & sparse).any()
    lab[six] = 5
    lab[sparse] = 3                    # ... but for `sparse`, which row 0 allows
    rows[0][sparse], rows[0][six] = True, False
    rows[1][six], rows[1][sparse] = True, False
    assert np.array_equal(np.flatnonzero(rows[0] & (lab == 3)), np.flatnonzero(sparse))
    assert np.array_equal(np.flatnonzero(rows[1] & (lab == 5)), np.sort(six))
    for half in (rows[0], rows[1], rows[2], lab == 3, lab == 5, (lab >= 1) & (lab <= 3)):
        assert int(half.sum()) > 5000
    assert int((rows[2] & (lab >= 1) & (lab <= 3)).sum()) > 5000
    return lab, rows


def three_path_triples():
    mo = np.tile(np.array([2, 0, 1, NONE]), 8)
    lo = np.tile(np.array([1, 3, 5, 0], dtype=np.uint32), 8)
    hi = np.tile(np.array([3, 3, 5, MAX], dtype=np.uint32), 8)
    return mo, lo, hi


def run_three_paths(index, ridx, mask_list, Q, deleted=(), what=""):
    lab, rows = three_path_halves(mask_list)
    mo, lo, hi = three_path_triples()
    conj, cmo = as_multi(30000, rows, lab, mo, lo, hi)
    pred = predicates(index, conj, deleted)
    # before the GPU runs: on the CPU, the sparse conjunction's walk fills the largest table, the dense one's ends well
    # within it -- path 2 and path 0 are not assumed
    allowed_s, a_sparse = pred(int(cmo[1]))
    assert 10 < a_sparse.size <= 16
    assert FR.graph(ridx, Q[1], 10, 64, allowed_s)["visited0"] > LIMIT
    g_dense = FR.graph(ridx, Q[0], 10, 64, pred(int(cmo[0]))[0])
    assert g_dense["visited0"] + g_dense["maxdeg0"] <= LIMIT
    index.set_labels(lab)
    s = index.mask_set(rows)
    try:
        index.search_batch_filtered_set_range(Q[:1], 10, 64, s, [NONE], 0, MAX)  # (uploads snapshot, set and column)
        before = stats_of(index, STATS + PATH_STATS)
        got, conj, cmo = both_and_multi(index, s, Q, 10, 64, rows, lab, mo, lo, hi, 10, what)
        d = delta(index, before)  # (the _multi call counts the same queries per path once more)
        assert np.array_equal(got[4], np.tile(np.array([0, 2, 1, 0], dtype=np.uint8), 8)), got[4]
        assert (d["filtered_queries_graph"], d["filtered_queries_exact"], d["filtered_overflow_exact"]) == (32, 16, 16)
        assert (d["filtered_set_range_calls"], d["filtered_set_range_groups"]) == (1, 4)
        assert d["filtered_set_calls"] == 0 and d["filtered_range_calls"] == 0
        assert d["label_words_uploaded"] == 0 and d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0
        sparse_rows = [qi for qi in range(32) if cmo[qi] == cmo[1]]
        check_rows(index, ridx, Q, 10, 64, conj, cmo, 10, got, deleted=deleted, what=what, skip=sparse_rows)
        for qi in sparse_rows:
            assert got[3][qi, 3] == 0
            compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_sparse), 10, (what, "sparse", qi))
        if deleted is not None and len(deleted):
            assert not np.isin(got[0], deleted).any()
    finally:
        s.close()
        index.set_option("filter_exact_max", 65536)


def test_three_paths_equal_multi_and_the_restatement(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    run_three_paths(index, ridx, mask_list, Q, what="three paths")


def test_three_paths_with_deleted_ids(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    rng = np.random.default_rng(84)
    deleted = np.concatenate([rng.choice(30000, 2000, replace=False), [77]])  # one of the six ids among them
    index.mark_deleted(deleted)
    try:
        run_three_paths(index, ridx, mask_list, Q, deleted=deleted, what="deleted")
    finally:
        index.unmark_deleted(deleted)


# ---- 2. every compiled form of the graph kernel reads both filters ------------------------------------------------------
def mixed_batch(nq, n_points, seed):
    """labels 0..4, three rows (the last one: only ids labelled 0) and a batch that mixes combined, row-only ([0, MAX]),
    range-only (HNSW_MASK_NONE), empty-range (lo > hi) and empty-intersection queries"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 5, size=n_points).astype(np.uint32)
    rows = np.stack([rng.random(n_points) < 0.5, rng.random(n_points) < 0.2, (lab == 0) & (rng.random(n_points) < 0.7)])
    kinds = [(0, 1, 2), (1, 0, 3), (0, 0, MAX), (NONE, 2, 3), (1, 4, 2), (2, 1, 4), (NONE, 0, MAX), (2, 0, 0), (1, 3, 3),
             (0, 4, 4)]
    mo = np.array([kinds[i % len(kinds)][0] for i in range(nq)])
    lo = np.array([kinds[i % len(kinds)][1] for i in range(nq)], dtype=np.uint32)
    hi = np.array([kinds[i % len(kinds)][2] for i in range(nq)], dtype=np.uint32)
    return lab, rows, mo, lo, hi


@pytest.mark.parametrize("kind,d", [(H.VEC_F32, 100), (H.VEC_F32, 128), (H.VEC_F32, 37), (H.VEC_QUANT8, 100),
                                    (H.VEC_QUANT8, 37)])
def test_shapes(kind, d):
    vs = rand_vectors(3000, d, 40 + d)
    qs = rand_vectors(30, d, 41 + d)
    index = H.HNSW.new(16, 64, d, kind).insert_bulk(vs, 4, False, levels=O.draw_levels(3000, 16, 2))
    index.set_option("filter_exact_max", -1)
    ridx = restated(index, vs)
    lab, rows, mo, lo, hi = mixed_batch(30, 3000, 50 + d)
    index.set_labels(lab)
    s = index.mask_set(rows)
    conj, cmo = as_multi(3000, rows, lab, mo, lo, hi)
    assert not conj[int(cmo[5])].any() and conj[int(cmo[7])].any()  # (row 2, [1, 4]): both halves allow ids, no id has both
    index.search_batch_filtered_set_range(qs[:2], 10, 64, s, mo[:2], lo[:2], hi[:2])  # (uploads snapshot, set, column)
    for (n, ef), r in (((10, 64), 1), ((64, 128), 2), ((64, 256), 4)):
        with H.kernel_log() as log:
            got = index.search_batch_filtered_set_range(qs, n, ef, s, mo, lo, hi)
        assert set(graph_kernels(log)) == {"hx_filt_graph_kernel<%s, %d>" % (FORMS[kind, d], r)}, dict(log)
        assert list(graph_kernels(log).values()) == [1] and "hx_filt_compact_kernel" not in log, dict(log)
        check_rows(index, ridx, qs, n, ef, conj, cmo, -1, got, what="d=%d n=%d ef=%d" % (d, n, ef))
        assert (got[4] == 0).all()
        for qi in (4, 5):  # the empty range and the empty intersection: count 0, status OK
            assert got[2][qi] == 0 and got[3][qi, 3] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
        same(got, index.search_batch_filtered_multi(qs, n, ef, conj, cmo), "d=%d n=%d ef=%d" % (d, n, ef))
    s.close()


# ---- 3. the compaction at its edges, exact path -------------------------------------------------------------------------
EDGE_IDS = np.array([0, 63, 64, 4095, 4096, 4129])


def edge_index(kind):
    vs = rand_vectors(4200, 8, 17)  # 66 mask words: a second block of 4096 ids, a partial last word
    index = H.HNSW.new(8, 32, 8, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(4200, 8, 5))
    return index, restated(index, vs), rand_vectors(6, 8, 18)


def check_exact(index, ridx, s, Q, rows_b, lab, mo, lo, hi, deleted, what):
    """all queries on the exact path with n = 64: against _multi and against the exact restatement under the conjunction"""
    got, conj, cmo = both_and_multi(index, s, Q, 64, 64, rows_b, lab, mo, lo, hi, 10 ** 9, what)
    assert (got[4] == 1).all(), (what, got[4])
    check_rows(index, ridx, Q, 64, 64, conj, cmo, 10 ** 9, got, deleted=deleted, what=what)
    return got, predicates(index, conj, deleted), cmo


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_compaction_edges_on_the_exact_path(kind):
    index, ridx, Q = edge_index(kind)
    rng = np.random.default_rng(19)
    for bits in (4130, 4300):  # allow_bits mid-word and below hnsw_len; then beyond it
        lab = rng.integers(0, 3, size=4200).astype(np.uint32)  # labels 0..2; the range below is [7, 9]
        row = rng.random(bits) < 0.5
        in_range = np.concatenate([EDGE_IDS, [4130, 100, 200, 4000, 4199]])  # their labels are in the range ...
        lab[in_range] = [7, 8, 9, 7, 8, 9, 7, 7, 8, 9, 7]
        row[EDGE_IDS] = True
        row[200] = True
        row[[100, 4000]] = False          # ... but these two have no bit,
        if bits > 4130:
            row[[4130, 4199]] = True      # (and beyond hnsw_len the row's bits name no id)
            row[4200:] = True
        rows_b = np.stack([row, rng.random(bits) < 0.3])
        index.set_labels(lab)
        s = index.mask_set(rows_b)
        assert s.allow_bits == bits
        deleted = np.array([64])          # one admissible id is deleted
        index.mark_deleted(deleted)
        try:
            mo = np.array([0, 0, 1, NONE, 0, 1])
            lo = np.array([7, 7, 0, 7, 0, 7], dtype=np.uint32)
            hi = np.array([9, 9, 1, 9, MAX, 6], dtype=np.uint32)
            got, pred, cmo = check_exact(index, ridx, s, Q, rows_b, lab, mo, lo, hi, deleted, "bits %d" % bits)
            want = [0, 63, 4095, 4096, 4129, 200] + ([4130, 4199] if bits > 4130 else [])
            assert sorted(pred(int(cmo[0]))[1].tolist()) == sorted(want)
            for qi in (0, 1):  # n = 64 >= A: every admissible id comes back, 4130 only when allow_bits reaches it
                assert sorted(got[0][qi][: got[2][qi]].tolist()) == sorted(want), (bits, got[0][qi])
            assert got[2][5] == 0  # an empty range next to them
        finally:
            index.unmark_deleted(deleted)
            s.close()


def test_labels_set_for_the_first_ids_only():
    index, ridx, Q = edge_index(H.VEC_F32)
    rng = np.random.default_rng(23)
    first = rng.integers(0, 4, size=100).astype(np.uint32)
    index.set_labels(first, np.arange(100))  # the rest read as 0
    lab = np.zeros(4200, dtype=np.uint32)
    lab[:100] = first
    rows_b = np.stack([rng.random(4200) < 0.5, rng.random(4200) < 0.02])
    s = index.mask_set(rows_b)
    mo = np.array([0, 0, 1, 1, NONE, NONE])
    lo = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint32)
    hi = np.array([0, MAX, 0, MAX, MAX, 0], dtype=np.uint32)
    got, pred, cmo = check_exact(index, ridx, s, Q, rows_b, lab, mo, lo, hi, (), "first 100")
    assert (pred(int(cmo[1]))[1] < 100).all() and got[2][1] == min(64, pred(int(cmo[1]))[1].size) > 0
    assert (got[0][3][: got[2][3]] < 100).all()
    index.set_option("filter_exact_max", -1)  # the graph path reads the same column
    got = index.search_batch_filtered_set_range(Q, 10, 64, s, mo, lo, hi)
    conj, cmo = as_multi(4200, rows_b, lab, mo, lo, hi)
    check_rows(index, ridx, Q, 10, 64, conj, cmo, -1, got, what="first 100, graph")
    s.close()


# ---- 4. one graph launch, one compaction per exact-path group, nothing uploaded or recounted twice ----------------------
def test_twenty_triples_one_launch_and_one_compaction_each(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(31)
    lab = (np.arange(1000) % 5).astype(np.uint32)
    rows_b = np.stack([rng.random(1000) < p for p in (0.6, 0.4, 0.2, 0.05)])
    index.set_labels(lab)
    s = index.mask_set(rows_b)
    Q = queries[:40]
    mo = np.arange(40) % 4
    lo = (np.arange(40) % 20 // 4).astype(np.uint32)
    hi = np.minimum(lo + (np.arange(40) % 4 == 3), 4).astype(np.uint32)
    conj, cmo = as_multi(1000, rows_b, lab, mo, lo, hi)
    assert len(conj) == 20
    sizes = sorted(int(m.sum()) for m in conj)
    cut = sizes[7]
    n_exact = sum(x <= cut for x in sizes)
    assert 0 < n_exact < 20
    index.set_option("filter_exact_max", cut)
    index.search_batch_filtered_set_range(Q[:1], 10, 64, s, [NONE], 0, MAX)  # (uploads snapshot, set and column)
    first = None
    for rep in range(2):
        before = stats_of(index, STATS)
        with H.kernel_log() as log:
            got = index.search_batch_filtered_set_range(Q, 10, 64, s, mo, lo, hi)
        d = delta(index, before)
        assert (d["filtered_set_range_calls"], d["filtered_set_range_groups"]) == (1, 20)
        assert d["label_words_uploaded"] == 0 and d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0
        # the planner reads the rows' own counts: each of the four is counted once, by the first call
        assert d["mask_set_recounts"] == (4 if rep == 0 else 0)
        assert d["mask_set_compactions"] == 0  # (no row's own list is made or used: every triple has a proper range)
        assert list(graph_kernels(log).values()) == [1], dict(log)
        assert log["hx_filt_compact_kernel"] == n_exact and log["hx_filt_merge_kernel"] == n_exact, dict(log)
        check_rows(index, ridx, Q, 10, 64, conj, cmo, cut, got, what="twenty triples")
        if first is not None:
            same(got, first, "second call")
        first = got
    same(first, index.search_batch_filtered_multi(Q, 10, 64, conj, cmo), "twenty triples")
    s.close()
    index.set_option("filter_exact_max", 65536)


# ---- 5. the set's caches survive a combined call ------------------------------------------------------------------------
def test_the_sets_caches_survive(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(37)
    lab = (np.arange(1000) % 5).astype(np.uint32)
    rows_b = np.stack([rng.random(1000) < p for p in (0.5, 0.03)])
    index.set_labels(lab)
    s = index.mask_set(rows_b)
    Q = queries[:20]
    mo = np.arange(20) % 2
    index.set_option("filter_exact_max", 100)  # row 1 (about 30 ids) is exact and gets its list; row 0 is not
    one = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    assert set(one[4].tolist()) == {0, 1}
    lo, hi = np.full(20, 1, dtype=np.uint32), np.full(20, 2, dtype=np.uint32)
    got, conj, cmo = both_and_multi(index, s, Q, 10, 64, rows_b, lab, mo, lo, hi, 100, "between")
    assert (got[4][mo == 1] == 1).all()  # the combined group under row 1 is exact too: compacted in the scratch
    check_rows(index, ridx, Q, 10, 64, conj, cmo, 100, got, what="between")
    before = stats_of(index, STATS)
    with H.kernel_log() as log:
        again = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    same(again, one, "the _set call after the combined call")
    d = delta(index, before)
    assert d["mask_set_recounts"] == 0 and d["mask_set_compactions"] == 0 and d["mask_set_words_uploaded"] == 0
    assert "hx_filt_compact_kernel" not in log, dict(log)  # row 1's list is still valid
    s.close()
    index.set_option("filter_exact_max", 65536)


# ---- 6. the degenerate equalities ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_max", [-1, 150])
def test_degenerate_equalities(glove, exact_max):
    index, ridx, queries = glove
    rng = np.random.default_rng(41)
    lab = (np.arange(1000) % 7).astype(np.uint32)
    rows_b = np.stack([rng.random(1000) < p for p in (0.5, 0.1, 0.0)])
    index.set_labels(lab)
    s = index.mask_set(rows_b)
    Q = queries[:30]
    mo = np.arange(30) % 4
    mo[mo == 3] = NONE
    index.set_option("filter_exact_max", exact_max)
    for n, ef in ((10, 64), (64, 100)):
        all_full = index.search_batch_filtered_set_range(Q, n, ef, s, mo, 0, MAX)
        same(all_full, index.search_batch_filtered_set(Q, n, ef, s, mo), "every range [0, MAX]")
        lo = (np.arange(30) % 7).astype(np.uint32)
        hi = (lo + np.arange(30) % 3).astype(np.uint32)
        lo[5], hi[5] = 4, 1
        all_none = index.search_batch_filtered_set_range(Q, n, ef, s, np.full(30, NONE), lo, hi)
        same(all_none, index.search_batch_filtered_range(Q, n, ef, lo, hi), "every row HNSW_MASK_NONE")
        if exact_max == 150:
            assert set(all_full[4].tolist()) == {0, 1} and set(all_none[4].tolist()) == {0, 1}
    row0 = index.search_batch_filtered_set_range(Q, 10, 64, s, None, 2, 4)  # mask_of None: row 0
    same(row0, index.search_batch_filtered_set_range(Q, 10, 64, s, np.zeros(30, dtype=np.int64), 2, 4), "row 0")
    s.close()
    index.set_option("filter_exact_max", 65536)


# ---- 7. the device form against the host form with filter_exact_max = -1 ---------------------------------------------
def test_device_form_equals_the_host_form(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    lab, rows = three_path_halves(mask_list)
    mo, lo, hi = three_path_triples()
    lo[[4, 13]], hi[[4, 13]] = 7, 2  # two empty ranges (d_lo > d_hi)
    index.set_labels(lab)
    s = index.mask_set(rows)
    index.set_option("filter_exact_max", -1)
    try:
        want = index.search_batch_filtered_set_range(Q, 10, 64, s, mo, lo, hi)
        assert set(want[4].tolist()) == {0, 2}  # the sparse and the six conjunctions are completed by the exact path
        assert (want[2][[4, 13]] == 0).all() and (want[3][[4, 13], 3] == 0).all()
        log = {}
        c0 = stats_of(index, STATS + PATH_STATS)
        code, dev = device_call(index, s, Q, 10, 64, mo, lo, hi, log_enqueue=log)
        assert code is None
        same(dev, want, "device form")
        assert list(graph_kernels(log).values()) == [1] and len(log) == 1, log  # the enqueue: ONE launch
        assert (dev[2][[4, 13]] == 0).all() and (dev[0][[4, 13]] == _lib.UINT32_MAX).all()
        d = delta(index, c0)
        assert d["filtered_set_range_calls"] == 1 and d["filtered_set_range_groups"] == 6 and d["filtered_queries_exact"] == 0
        assert d["filtered_set_calls"] == 0 and d["filtered_range_calls"] == 0
        assert d["filtered_overflow_exact"] == int((want[4] == 2).sum()) > 0
        assert d["filtered_queries_graph"] == 32 - d["filtered_overflow_exact"]
        assert d["label_words_uploaded"] == 0 and d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0
        code, dev = device_call(index, s, Q, 10, 64, mo, lo, hi, optional=False)  # without d_dists and d_counts
        assert code is None and np.array_equal(dev[0], want[0]) and np.array_equal(dev[3], want[3])
        assert np.array_equal(dev[4], want[4])
        # d_mask_of NULL: every query under row 0
        want0 = index.search_batch_filtered_set_range(Q, 10, 64, s, np.zeros(32, dtype=np.int64), lo, hi)
        code, dev = device_call(index, s, Q, 10, 64, None, lo, hi)
        assert code is None
        same(dev, want0, "device form, d_mask_of NULL")
        # a row the set does not have: that query's own error, the others as before
        bad = mo.copy()
        bad[[6, 21]] = [3, 1000]
        code, dev = device_call(index, s, Q, 10, 64, bad, lo, hi)
        assert code == _lib.ERR_ARG
        ok = np.setdiff1d(np.arange(32), [6, 21])
        for k in range(4):
            a, b = dev[k][ok], want[k][ok]
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b), k
        for qi in (6, 21):
            assert dev[3][qi].tolist() == [0, 0, 0, _lib.ERR_ARG & 0xFFFFFFFF], dev[3][qi]
            assert dev[2][qi] == 0 and (dev[0][qi] == _lib.UINT32_MAX).all()
            assert np.isinf(dev[1][qi]).all()
    finally:
        s.close()
        index.set_option("filter_exact_max", 65536)


# ---- 8. a NaN query; the cosine option; ef' above the graph path's limit; later inserts --------------------------------
@pytest.mark.parametrize("exact_max", [-1, 60])
def test_a_nan_query_is_its_own_error(glove, exact_max):
    index, ridx, queries = glove
    rng = np.random.default_rng(43)
    lab = (np.arange(1000) % 7).astype(np.uint32)
    rows_b = np.stack([rng.random(1000) < p for p in (0.6, 0.3)])
    index.set_labels(lab)
    s = index.mask_set(rows_b)
    Q = queries[:24].copy()
    mo = np.arange(24) % 3
    mo[mo == 2] = NONE
    lo = (np.arange(24) % 7).astype(np.uint32)
    hi = (lo + np.arange(24) % 2).astype(np.uint32)
    Q[9, 4] = np.nan   # (row 0, [2, 2]): about 85 ids, the graph path under both settings
    Q[19, 0] = np.nan  # (row 1, [5, 5]): about 43 ids, the exact path under 60
    lo[9], hi[9], lo[19], hi[19] = 2, 2, 5, 5
    index.set_option("filter_exact_max", exact_max)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_set_range(Q, 10, 64, s, mo, lo, hi)
    assert e.value.code == _lib.ERR_NAN_INPUT
    rc, got = raw_both(index, s, Q, 10, 64, mo, lo, hi)
    conj, cmo = as_multi(1000, rows_b, lab, mo, lo, hi)
    rc_m, want = raw_multi(index, Q, 10, 64, conj, cmo)
    assert rc == rc_m == _lib.ERR_NAN_INPUT
    same(got, want, "nan")
    assert int(conj[int(cmo[19])].sum()) <= 60 < int(conj[int(cmo[9])].sum())
    assert got[4][19] == (1 if exact_max == 60 else 0) and got[4][9] == 0
    for qi in (9, 19):
        assert got[3][qi, 3] == _lib.ERR_NAN_INPUT and got[2][qi] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
    check_rows(index, ridx, Q, 10, 64, conj, cmo, exact_max, got, what="nan", skip=(9, 19))
    if exact_max == -1:  # the device form reports the same rows and the same first error
        code, dev = device_call(index, s, Q, 10, 64, mo, lo, hi)
        assert code == _lib.ERR_NAN_INPUT
        same(dev[:4], (got[0], got[1], got[2], got[3].view(np.uint64).astype(np.uint32).astype(np.int64)), "device nan")
    s.close()
    index.set_option("filter_exact_max", 65536)


def test_cosine_option():
    d = 32
    vs = rand_vectors(2000, d, 91) - np.float32(0.5)
    qs = rand_vectors(20, d, 92) - np.float32(0.5)
    index = H.HNSW.new(12, 48, d, H.VEC_F32)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 2, False, levels=O.draw_levels(2000, 12, 4))

    def unit(x):
        s = np.zeros(x.shape[0], dtype=np.float32)
        for e in range(x.shape[1]):
            s = s + x[:, e] * x[:, e]
        return x / np.sqrt(s)[:, None]

    stored = np.stack([index.get_point(i).get_vals() for i in range(2000)])
    ridx = restated(index, stored)
    rng = np.random.default_rng(93)
    lab = rng.integers(0, 20, size=2000).astype(np.uint32)
    rows_b = np.stack([rng.random(2000) < 0.5, rng.random(2000) < 0.25])
    index.set_labels(lab)
    s = index.mask_set(rows_b)
    mo = np.arange(20) % 2
    lo = np.array([i % 5 for i in range(20)], dtype=np.uint32)
    hi = (lo + np.array([0, 5, 14] * 7)[:20]).astype(np.uint32)
    for exact_max in (-1, 150):
        got, conj, cmo = both_and_multi(index, s, qs, 10, 64, rows_b, lab, mo, lo, hi, exact_max, "cosine %d" % exact_max)
        check_rows(index, ridx, qs, 10, 64, conj, cmo, exact_max, got, what="cosine", Qr=unit(qs))
        assert (got[4] == 1).any() == (exact_max == 150)
    index.set_option("filter_exact_max", -1)
    want = index.search_batch_filtered_set_range(qs, 10, 64, s, mo, lo, hi)
    code, dev = device_call(index, s, qs, 10, 64, mo, lo, hi)
    assert code is None
    same(dev, want, "device form, cosine")
    s.close()


def test_ef_above_the_graph_paths_limit(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(47)
    index.set_labels((np.arange(1000) % 7).astype(np.uint32))
    rows_b = np.stack([rng.random(1000) < 0.5, rng.random(1000) < 0.9])
    s = index.mask_set(rows_b)
    Q = queries[:8]
    index.set_option("filter_exact_max", 200)  # one label under a row: at most 143 ids, exact; three labels under row 1: graph
    try:
        got = index.search_batch_filtered_set_range(Q, 10, 257, s, [0, 1] * 4, 2, 2)  # exact-path triples only: allowed
        assert (got[4] == 1).all()
        for n, ef in ((10, 257), (1, 1000)):
            with pytest.raises(H.HnswError) as e:
                index.search_batch_filtered_set_range(Q, n, ef, s, [0, 0, 0, 0, 0, 0, 0, 1], [2] * 8, [2] * 7 + [4])
            assert e.value.code == _lib.ERR_ARG, (n, ef)
    finally:
        s.close()
        index.set_option("filter_exact_max", 65536)


def test_after_insert_vec_the_new_id_has_label_zero():
    d, n0 = 24, 1500
    vs = rand_vectors(n0, d, 61)
    index = H.HNSW.new(8, 32, d, H.VEC_QUANT8).insert_bulk(vs, 2, False, levels=O.draw_levels(n0, 8, 3))
    index.search_batch(vs[:2], 10, 32)  # (uploads the snapshot)
    lab = (np.arange(n0) % 2).astype(np.uint32)
    index.set_labels(lab)
    tight = index.mask_set([np.ones(n0, dtype=bool)])           # made without spare bits
    roomy = index.mask_set(np.zeros((1, n0 + 100), dtype=bool))  # room for later ids
    roomy.update(0, np.arange(0, n0, 3))
    qs = rand_vectors(4, d, 63)
    for s in (tight, roomy):
        index.search_batch_filtered_set_range(qs, 10, 32, s, None, 0, 0)  # (set and column go to HBM before the insert)
    new = rand_vectors(1, d, 62)[0]
    assert index.insert_vec(new, level=0) == n0
    assert index.get_labels([n0]).tolist() == [0]
    ridx = restated(index, np.concatenate([vs, new[None, :]]))
    lab1 = np.concatenate([lab, [0]]).astype(np.uint32)
    Q = np.concatenate([new[None, :], qs])
    for exact_max in (-1, 10 ** 9):
        # label 0, but outside a set made without spare bits ...
        got, conj, cmo = both_and_multi(index, tight, Q, 10, 32, [np.ones(n0, dtype=bool)], lab1, np.zeros(5, dtype=np.int64),
                                        np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32), exact_max, "tight")
        assert n0 not in got[0]
        check_rows(index, ridx, Q, 10, 32, conj, cmo, exact_max, got, what="tight")
    # ... and admissible under [0, 0] once a set with spare bits allows it
    roomy.update(0, [n0])
    row = np.zeros(n0 + 100, dtype=bool)
    row[np.arange(0, n0, 3)] = True
    row[n0] = True
    for exact_max in (-1, 10 ** 9):
        got, conj, cmo = both_and_multi(index, roomy, Q, 10, 32, [row], lab1, np.zeros(5, dtype=np.int64),
                                        np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32), exact_max, "roomy")
        assert n0 in got[0][0], got[0][0]
        check_rows(index, ridx, Q, 10, 32, conj, cmo, exact_max, got, what="roomy")
        assert n0 not in index.search_batch_filtered_set_range(Q, 10, 32, roomy, None, 1, 1)[0]
    assert index.stat("point_patches") == 1 and index.stat("patch_fallbacks") == 0
    tight.close()
    roomy.close()
