"""Resident mask sets on the MI355X: hnsw_search_batch_filtered_set against hnsw_search_batch_filtered_multi (ids,
distance bits, counts, stats, paths) and against the CPU restatement under every row's own predicate; what stays in HBM
between calls (uploads, recounts, compactions, launches); the device-pointer form against the host form with
filter_exact_max = -1, its in-kernel check of d_mask_of included; the lists' budget."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import LIMIT, _import_graph, restated
from tests.test_gpu_filtered_multi import (NONE, check_rows, compare_row, dealt, glove, graph_kernels,  # noqa: F401
                                           predicates, raw_multi)
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

SET_STATS = ("mask_set_words_uploaded", "mask_set_recounts", "mask_set_compactions", "filtered_set_calls")
PATH_STATS = ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact")


def stats_of(index, keys=SET_STATS + PATH_STATS):
    return {k: index.stat(k) for k in keys}


def delta(index, before):
    return {k: index.stat(k) - v for k, v in before.items()}


def same(a, b, what=""):
    """two results (ids, dists, counts, stats, paths): equal bit for bit"""
    for name, x, y in zip(("ids", "dists", "counts", "stats", "paths"), a, b):
        x = x.view(np.uint32) if x.dtype == np.float32 else x
        y = y.view(np.uint32) if y.dtype == np.float32 else y
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:5])


def as_bool(mask_list, bits):
    """the masks of a call as bool rows over `bits` ids (what a set is made from and updated against)"""
    out = np.zeros((len(mask_list), bits), dtype=bool)
    for g, m in enumerate(mask_list):
        m = np.asarray(m)
        if m.dtype == np.bool_:
            out[g, : m.shape[0]] = m
        else:
            out[g, m] = True
    return out


def set_and_multi(index, s, Q, n, ef, mask_list, mo, exact_max, what=""):
    """the call under the set and the same call with the masks passed along: equal; -> the set's result"""
    index.set_option("filter_exact_max", exact_max)
    got = index.search_batch_filtered_set(Q, n, ef, s, mo)
    want = index.search_batch_filtered_multi(Q, n, ef, mask_list, mo)
    same(got, want, what)
    return got


def raw_set(index, Q, n, ef, s, mask_of):
    """the C entry itself -> status and the five arrays (the Python mirror raises on a per-query error)"""
    mo = np.where(np.asarray(mask_of) < 0, H.MASK_NONE, mask_of).astype(np.uint32)
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    ids = np.full((nq, n), _lib.UINT32_MAX, dtype=np.uint32)
    dists = np.full((nq, n), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    stats = np.zeros((nq, 4), dtype=np.int32)
    paths = np.zeros(nq, dtype=np.uint8)

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    rc = _lib.lib().hnsw_search_batch_filtered_set(
        index._h, p(Q, C.c_float), nq, n, ef, s._s, p(mo, C.c_uint32), p(ids, C.c_uint32), p(dists, C.c_float),
        p(counts, C.c_uint32), C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)), p(paths, C.c_uint8))
    return rc, (ids, dists, counts, stats.astype(np.int64), paths)


def device_call(index, s, Q, n, ef, mo, optional=True, log_enqueue=None):
    """the device form with torch tensors in HBM, completed by _finish -> (status or None, the five arrays)"""
    import torch
    dev = torch.device("cuda:0")
    nq = Q.shape[0]
    dQ = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    d_mo = None
    if mo is not None:
        d_mo = torch.from_numpy(np.where(np.asarray(mo) < 0, H.MASK_NONE, mo).astype(np.uint32).view(np.int32)).to(dev)
    d_ids = torch.zeros((nq, n), dtype=torch.int32, device=dev)
    d_d = torch.zeros((nq, n), dtype=torch.float32, device=dev)
    d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_s = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    args = (dQ.data_ptr(), nq, n, ef, s, 0 if d_mo is None else d_mo.data_ptr(), d_ids.data_ptr(),
            d_d.data_ptr() if optional else 0, d_c.data_ptr() if optional else 0, d_s.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    if log_enqueue is not None:
        with H.kernel_log() as log:
            index.search_batch_filtered_device(*args)
        log_enqueue.update(log)
    else:
        index.search_batch_filtered_device(*args)
    code = None
    paths = np.zeros(nq, dtype=np.uint8)
    try:
        paths = index.search_batch_filtered_device_finish(*args, paths=True)
    except H.HnswError as e:
        code = e.code
    torch.cuda.synchronize(dev)
    return code, (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                  d_s.cpu().numpy().view(np.uint32).astype(np.int64), paths)


# ---- 1. equality with _multi and with the restatement, all three paths in one call -------------------------------
@pytest.fixture(scope="module", params=[H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def three_paths(request):
    """the index and the masks of test_graph_exact_and_overflow_paths_in_one_call: a dense random graph over 30000
    points; `dense` ends the walk early (path 0), `sparse` makes it fill the largest table (2), `six` is exact (1)"""
    n, d = 30000, 8
    vs = rand_vectors(n, d, 81)
    rng = np.random.default_rng(82)
    nbrs = rng.integers(0, n, size=(n, 12))
    rows = [set() for _ in range(n)]
    for i in range(n):
        for j in nbrs[i].tolist():
            if j != i:
                rows[i].add(j)
                rows[j].add(i)
    index = _import_graph(vs, request.param, 8, rows)
    ridx = restated(index, vs)
    sparse = rng.random(n) < 0.0005
    dense = rng.random(n) < 0.5
    assert int(sparse.sum()) == 16
    six = np.array([3, 77, 4096, 12345, 20000, 29999])
    qs = rand_vectors(8, d, 83)
    Q = np.repeat(qs, 4, axis=0)
    mo = np.tile(np.array([0, 1, 2, NONE]), 8)
    return index, ridx, [dense, sparse, six], Q, mo


def check_three_paths(index, ridx, mask_list, Q, mo, got, deleted=(), what=""):
    """every path occurs; every row against the restatement under its own predicate (the sparse rows, whose walk
    fills the largest table, against the exact restatement)"""
    paths = got[4]
    assert all((paths == p).any() for p in (0, 1, 2)), paths
    sparse_rows = [qi for qi in range(Q.shape[0]) if mo[qi] == 1]
    assert (paths[sparse_rows] == 2).all(), paths
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, 10, got, deleted=deleted, what=what, skip=sparse_rows)
    allowed, a_ids = predicates(index, mask_list, deleted)(1)
    assert FR.graph(ridx, Q[sparse_rows[0]], 10, 64, allowed)["visited0"] > LIMIT
    for qi in sparse_rows:
        assert got[3][qi, 3] == 0
        compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_ids), 10, (what, "sparse", qi))


def test_three_paths_equal_multi_and_the_restatement(three_paths):
    index, ridx, mask_list, Q, mo = three_paths
    s = index.mask_set(mask_list)
    assert (s.n_masks, s.allow_bits) == (3, 30000)
    before = stats_of(index)
    got = set_and_multi(index, s, Q, 10, 64, mask_list, mo, 10, "three paths")
    assert np.array_equal(got[4], np.tile(np.array([0, 2, 1, 0], dtype=np.uint8), 8)), got[4]
    d = delta(index, before)  # (the _multi call counts the same queries per path once more)
    assert (d["filtered_queries_graph"], d["filtered_queries_exact"], d["filtered_overflow_exact"]) == (32, 16, 16)
    assert d["filtered_set_calls"] == 1 and d["mask_set_recounts"] == 3
    check_three_paths(index, ridx, mask_list, Q, mo, got, what="three paths")
    # the device form: what the set gives with filter_exact_max = -1 (the six ids by the graph path too), paths 0 / 2
    index.set_option("filter_exact_max", -1)
    want = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    assert set(want[4].tolist()) == {0, 2}
    log = {}
    c0 = stats_of(index)
    code, dev = device_call(index, s, Q, 10, 64, mo, log_enqueue=log)
    assert code is None
    same(dev, want, "device form, three paths")
    assert list(graph_kernels(log).values()) == [1] and len(log) == 1, log
    d = delta(index, c0)
    assert d["filtered_set_calls"] == 1 and d["filtered_queries_exact"] == 0
    assert d["filtered_overflow_exact"] == int((want[4] == 2).sum()) > 0
    assert d["filtered_queries_graph"] == 32 - d["filtered_overflow_exact"]
    s.close()


def test_three_paths_with_deleted_ids(three_paths):
    index, ridx, mask_list, Q, mo = three_paths
    s = index.mask_set(mask_list)
    rng = np.random.default_rng(84)
    deleted = np.concatenate([rng.choice(30000, 2000, replace=False), [77]])  # one of the six ids among them
    index.search_batch_filtered_set(Q[:4], 10, 64, s, mo[:4])
    index.mark_deleted(deleted)
    try:
        before = stats_of(index)
        got = set_and_multi(index, s, Q, 10, 64, mask_list, mo, 10, "deleted")
        d = delta(index, before)
        assert d["mask_set_words_uploaded"] == 0 and d["mask_set_recounts"] == 3
        assert not np.isin(got[0], deleted).any()
        check_three_paths(index, ridx, mask_list, Q, mo, got, deleted=deleted, what="deleted")
        index.set_option("filter_exact_max", -1)
        want = index.search_batch_filtered_set(Q, 10, 64, s, mo)
        code, dev = device_call(index, s, Q, 10, 64, mo, optional=False)
        assert code is None and np.array_equal(dev[0], want[0]) and np.array_equal(dev[3], want[3])
        assert np.array_equal(dev[4], want[4]) and not np.isin(dev[0], deleted).any()
    finally:
        index.unmark_deleted(deleted)
        s.close()


def check_all_path_2(index, ridx, mask_list, Q, mo, got, deleted, sizes, what):
    """every query took path 2: the walk under the first key, restated, fills the largest table, and every row is the
    exact restatement's under its own key"""
    assert (got[4] == 2).all(), (what, got[4])
    pred = predicates(index, mask_list, deleted)
    for k, (g, size) in enumerate(sizes):
        allowed, a_ids = pred(g)
        assert a_ids.size == size, (what, g, a_ids.size)
        rows = np.flatnonzero(mo == g)
        if k == 0:
            assert FR.graph(ridx, Q[rows[0]], 10, 64, allowed)["visited0"] > LIMIT
        for qi in rows:
            assert got[3][qi, 3] == 0
            compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_ids), 10, (what, qi))


def test_path_2_under_two_keys_in_one_call(three_paths):
    """with filter_exact_max = -1 the queries under `six` fill the largest table as those under `sparse` do: path 2 row
    by row in _multi, under the set and in the device form, where `six` has its list in the set and `sparse` has not"""
    index, ridx, mask_list, Q, _ = three_paths
    Q8, mo = Q[::4], np.tile(np.array([1, 2]), 4)
    s = index.mask_set(mask_list)
    index.set_option("filter_exact_max", 10)
    index.search_batch_filtered_set(Q8, 10, 64, s, mo)  # (`six` is planned exact: its list is made in the set)
    before = stats_of(index)
    got = set_and_multi(index, s, Q8, 10, 64, mask_list, mo, -1, "two keys")
    d = delta(index, before)  # (the _multi call counts the same queries once more)
    assert (d["filtered_queries_graph"], d["filtered_queries_exact"], d["filtered_overflow_exact"]) == (0, 0, 16)
    assert d["mask_set_compactions"] == 1 and d["mask_set_recounts"] == 0  # `sparse`, in the scratch
    check_all_path_2(index, ridx, mask_list, Q8, mo, got, (), ((2, 6), (1, 16)), "two keys")
    for optional in (True, False):  # ... and without d_dists and d_counts
        before = stats_of(index)
        with H.kernel_log() as log:
            code, dev = device_call(index, s, Q8, 10, 64, mo, optional=optional)
        assert code is None
        same(dev if optional else dev[:1] + got[1:3] + dev[3:], got, "device form, two keys")
        d = delta(index, before)
        assert d["filtered_overflow_exact"] == 8 and d["mask_set_compactions"] == 1 and d["mask_set_recounts"] == 0
        assert log["hx_filt_compact_kernel"] == 1, dict(log)
    s.close()


def test_path_2_without_a_mask_next_to_a_row(three_paths):
    """with all but 20 ids deleted the walk of a query without a mask fills the largest table too: HNSW_MASK_NONE and
    the sparse row on path 2 in one call, in _multi, under the set and in the device form"""
    index, ridx, mask_list, Q, _ = three_paths
    keep = np.union1d(np.flatnonzero(mask_list[1]), [5, 1000, 15000, 29000])
    assert keep.size == 20
    deleted = np.setdiff1d(np.arange(30000), keep)
    Q8, mo = Q[::4], np.tile(np.array([NONE, 1]), 4)
    s = index.mask_set(mask_list)
    index.mark_deleted(deleted)
    try:
        before = stats_of(index)
        got = set_and_multi(index, s, Q8, 10, 64, mask_list, mo, -1, "no mask next to a row")
        d = delta(index, before)
        assert (d["filtered_queries_graph"], d["filtered_queries_exact"], d["filtered_overflow_exact"]) == (0, 0, 16)
        check_all_path_2(index, ridx, mask_list, Q8, mo, got, deleted, ((NONE, 20), (1, 16)), "no mask next to a row")
        code, dev = device_call(index, s, Q8, 10, 64, mo)
        assert code is None
        same(dev, got, "device form, no mask next to a row")
    finally:
        index.unmark_deleted(deleted)
        s.close()
        index.set_option("filter_exact_max", 65536)


# ---- 2. the other cases of the contract --------------------------------------------------------------------------
@pytest.mark.parametrize("exact_max", [-1, 50])
def test_reference_test_data_with_none_rows(glove, exact_max):
    from tests.test_gpu_filtered import masks
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    s = index.mask_set(mask_list)
    mo = dealt(40, 6, none_at=(7, 19, 33))
    for n, ef in ((10, 64), (1, 1), (64, 100), (10, 256)):
        got = set_and_multi(index, s, queries[:40], n, ef, mask_list, mo, exact_max, "n=%d ef=%d" % (n, ef))
        check_rows(index, ridx, queries[:40], n, ef, mask_list, mo, exact_max, got, what="set n=%d ef=%d" % (n, ef))
    # mask_of None: every query under row 0
    got = index.search_batch_filtered_set(queries[:40], 10, 64, s)
    same(got, index.search_batch_filtered_multi(queries[:40], 10, 64, mask_list, np.zeros(40, dtype=np.int64)), "row 0")
    if exact_max == 50:  # ef' > 256 is refused only when a named row takes the graph path
        few = np.where(mo == NONE, 3, np.where(mo < 3, 3, mo))
        got = set_and_multi(index, s, queries[:40], 10, 300, mask_list, few, 50, "ef 300, exact rows only")
        assert (got[4] == 1).all()
        with pytest.raises(H.HnswError) as e:
            index.search_batch_filtered_set(queries[:40], 10, 300, s, mo)
        assert e.value.code == _lib.ERR_ARG


def test_after_insert_vec_the_new_id_is_allowed_by_update():
    d = 24
    vs = rand_vectors(1500, d, 61)
    index = H.HNSW.new(8, 32, d, H.VEC_QUANT8).insert_bulk(vs, 2, False, levels=O.draw_levels(1500, 8, 3))
    index.upload()
    rng = np.random.default_rng(64)
    bits = 1600  # room for the ids of later inserts
    masks_b = as_bool([np.ones(1500, dtype=bool), rng.random(1500) < 0.2], bits)
    s = index.mask_set(masks_b)
    assert s.allow_bits == bits > index.len()
    qs0 = rand_vectors(10, d, 63)
    mo0 = dealt(10, 2, none_at=(3,))
    index.search_batch_filtered_set(qs0, 10, 32, s, mo0)  # (the set goes to HBM before the inserts)
    new = rand_vectors(40, d, 62)
    for v in new:
        index.insert_vec(v, level=0)
    assert index.stat("point_patches") == 40 and index.stat("patch_fallbacks") == 0
    ridx = restated(index, np.concatenate([vs, new]))
    qs = np.concatenate([new[:8], qs0])
    mo = dealt(18, 2, none_at=(0, 3, 5, 6, 11, 16))
    for exact_max in (-1, 400):
        got = set_and_multi(index, s, qs, 10, 32, list(masks_b), mo, exact_max, "patched")
        check_rows(index, ridx, qs, 10, 32, list(masks_b), mo, exact_max, got, what="patched")
        found = got[0][mo != NONE]
        assert (found[found != _lib.UINT32_MAX] < 1500).all()  # the rows made before the inserts leave the new points out
    # ... until update allows them: the new ids in row 1, found by the queries that are those points
    new_ids = np.arange(1500, 1540)
    before = stats_of(index, SET_STATS)
    s.update(1, new_ids)
    masks_b[1, new_ids] = True
    assert np.array_equal(s.read(1), H.pack_allow(masks_b[1])[0])
    for exact_max in (-1, 400):
        got = set_and_multi(index, s, qs, 10, 32, list(masks_b), mo, exact_max, "patched and updated")
        check_rows(index, ridx, qs, 10, 32, list(masks_b), mo, exact_max, got, what="patched and updated")
        found = got[0][mo == 1]
        assert ((found >= 1500) & (found != _lib.UINT32_MAX)).any()
        found = got[0][mo == 0]
        assert (found[found != _lib.UINT32_MAX] < 1500).all()
    d_ = delta(index, before)
    assert d_["mask_set_words_uploaded"] == 2 and d_["mask_set_recounts"] == 1  # ids 1500..1539 lie in two words
    assert index.stat("point_patches") == 40 and index.stat("patch_fallbacks") == 0


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
    mask_list = [rng.random(2000) < 0.3, rng.random(2000) < 0.05, rng.random(2000) < 0.6]
    s = index.mask_set(mask_list)
    mo = dealt(20, 3, none_at=(5, 12))
    for exact_max in (-1, 300):
        got = set_and_multi(index, s, qs, 10, 64, mask_list, mo, exact_max, "cosine %d" % exact_max)
        check_rows(index, ridx, qs, 10, 64, mask_list, mo, exact_max, got, what="cosine", Qr=unit(qs))
    index.set_option("filter_exact_max", -1)
    want = index.search_batch_filtered_set(qs, 10, 64, s, mo)
    code, dev = device_call(index, s, qs, 10, 64, mo)
    assert code is None
    same(dev, want, "device form, cosine")


@pytest.mark.parametrize("exact_max", [-1, 50])
def test_a_nan_query_is_its_own_error(glove, exact_max):
    from tests.test_gpu_filtered import masks
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    s = index.mask_set(mask_list)
    mo = dealt(24, 6, none_at=(8,))
    Q = queries[:24].copy()
    Q[9, 4] = np.nan   # a query of "0.01": the graph path under -1, the exact path under 50
    Q[20, 0] = np.nan  # a query of "0.1": the graph path under both
    index.set_option("filter_exact_max", exact_max)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_set(Q, 10, 64, s, mo)
    assert e.value.code == _lib.ERR_NAN_INPUT
    rc, got = raw_set(index, Q, 10, 64, s, mo)
    rc_m, want = raw_multi(index, Q, 10, 64, mask_list, mo)
    assert rc == rc_m == _lib.ERR_NAN_INPUT
    same(got, want, "nan")
    for qi in (9, 20):
        assert got[3][qi, 3] == _lib.ERR_NAN_INPUT and got[2][qi] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, exact_max, got, what="nan", skip=(9, 20))
    if exact_max == -1:  # the device form reports the same rows and the same first error
        code, dev = device_call(index, s, Q, 10, 64, mo)
        assert code == _lib.ERR_NAN_INPUT
        same(dev[:4], (got[0], got[1], got[2], got[3].view(np.uint64).astype(np.uint32).astype(np.int64)), "device nan")


# ---- 3. residency: what a call under a set does not do again --------------------------------------------------------
def test_residency(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(31)
    G, W = 8, (1000 + 63) // 64
    masks_b = rng.random((G, 1000)) < 0.3
    Q = np.concatenate([queries, queries])[:64]
    mo = dealt(64, G)
    index.search_batch(Q[:2], 10, 64)  # (uploads the snapshot)
    for exact_max, n_graph in ((10 ** 9, 0), (-1, 1)):
        index.set_option("filter_exact_max", exact_max)
        s = index.mask_set(masks_b)
        # the first call: the whole set goes up, every named row is counted (and compacted on the exact path)
        before = stats_of(index, SET_STATS)
        with H.kernel_log() as log:
            first = index.search_batch_filtered_set(Q, 10, 64, s, mo)
        assert delta(index, before) == {"mask_set_words_uploaded": G * W, "mask_set_recounts": G,
                                        "mask_set_compactions": 0 if n_graph else G, "filtered_set_calls": 1}
        assert log.get("hx_filt_compact_kernel", 0) == (0 if n_graph else G), dict(log)
        assert "hx_deleted_scatter_kernel" not in log
        assert list(graph_kernels(log).values()) == [1] * n_graph, dict(log)  # one launch, however many rows
        same(first, index.search_batch_filtered_multi(Q, 10, 64, list(masks_b), mo), "first call")
        check_rows(index, ridx, Q, 10, 64, list(masks_b), mo, exact_max, first, what="first call")
        # the identical second call: nothing goes up, nothing is counted, nothing is compacted
        before = stats_of(index, SET_STATS)
        with H.kernel_log() as log:
            second = index.search_batch_filtered_set(Q, 10, 64, s, mo)
        assert delta(index, before) == {"mask_set_words_uploaded": 0, "mask_set_recounts": 0,
                                        "mask_set_compactions": 0, "filtered_set_calls": 1}
        assert "hx_filt_compact_kernel" not in log and "hx_deleted_scatter_kernel" not in log, dict(log)
        assert log.get("hx_filt_merge_kernel", 0) == (0 if n_graph else G), dict(log)
        assert list(graph_kernels(log).values()) == [1] * n_graph, dict(log)
        same(second, first, "second call")
        # an update of ids in w = 3 distinct words of one row (3 < G W / 8): exactly those words travel, by one scatter
        ids = np.array([5, 6, 70, 130, 131, 190])  # words 0, 1, 2
        on = ~masks_b[2, ids]  # (the two updates below toggle all six)
        masks2 = masks_b.copy()
        masks2[2, ids] = on
        s.update(2, ids[on])
        s.update(2, ids[~on], allow=False)
        before = stats_of(index, SET_STATS)
        with H.kernel_log() as log:
            third = index.search_batch_filtered_set(Q, 10, 64, s, mo)
        assert delta(index, before) == {"mask_set_words_uploaded": 3, "mask_set_recounts": 1,
                                        "mask_set_compactions": 0 if n_graph else 1, "filtered_set_calls": 1}
        assert log["hx_deleted_scatter_kernel"] == 1 and log.get("hx_filt_compact_kernel", 0) == (0 if n_graph else 1)
        same(third, index.search_batch_filtered_multi(Q, 10, 64, list(masks2), mo), "after update")
        check_rows(index, ridx, Q, 10, 64, list(masks2), mo, exact_max, third, what="after update")
        # ... and a call that does not name the row counts nothing (the words still travel)
        s.update(2, [999])
        masks2[2, 999] = True
        before = stats_of(index, SET_STATS)
        mo_not2 = np.where(mo == 2, 3, mo)
        index.search_batch_filtered_set(Q, 10, 64, s, mo_not2)
        assert delta(index, before) == {"mask_set_words_uploaded": 1, "mask_set_recounts": 0,
                                        "mask_set_compactions": 0, "filtered_set_calls": 1}
        # deletions: no word of the set travels, every named row is counted again, no result holds a deleted id
        deleted = rng.choice(1000, 100, replace=False)
        index.mark_deleted(deleted)
        try:
            before = stats_of(index, SET_STATS)
            with H.kernel_log() as log:
                fourth = index.search_batch_filtered_set(Q, 10, 64, s, mo)
            assert delta(index, before) == {"mask_set_words_uploaded": 0, "mask_set_recounts": G,
                                            "mask_set_compactions": 0 if n_graph else G, "filtered_set_calls": 1}
            assert list(graph_kernels(log).values()) == [1] * n_graph, dict(log)
            assert not np.isin(fourth[0], deleted).any()
            same(fourth, index.search_batch_filtered_multi(Q, 10, 64, list(masks2), mo), "deleted")
            check_rows(index, ridx, Q, 10, 64, list(masks2), mo, exact_max, fourth, deleted=deleted, what="deleted")
        finally:
            index.unmark_deleted(deleted)
        s.close()
    index.set_option("filter_exact_max", 65536)


def test_a_large_update_is_one_whole_copy(glove):
    index, ridx, queries = glove
    index.set_option("filter_exact_max", 65536)
    G, W = 4, 16
    masks_b = np.zeros((G, 1000), dtype=bool)
    s = index.mask_set(masks_b)
    Q, mo = queries[:8], dealt(8, G)
    index.search_batch_filtered_set(Q, 10, 64, s, mo)
    ids = np.arange(0, 64 * 9, 64)  # 9 words of 64: more than an eighth
    s.update(1, ids)
    masks_b[1, ids] = True
    before = stats_of(index, SET_STATS)
    with H.kernel_log() as log:
        got = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    assert delta(index, before)["mask_set_words_uploaded"] == G * W and "hx_deleted_scatter_kernel" not in log
    same(got, index.search_batch_filtered_multi(Q, 10, 64, list(masks_b), mo), "whole copy")


# ---- 4. the device form --------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(glove):
    from tests.test_gpu_filtered import masks
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    s = index.mask_set(mask_list)
    Q = queries[:40]
    mo = dealt(40, 6, none_at=(7, 19, 33))
    index.set_option("filter_exact_max", -1)
    deleted = np.arange(0, 1000, 7)
    for dele in ((), deleted):
        if len(dele):
            index.mark_deleted(dele)
        try:
            for n, ef in ((10, 64), (1, 1), (64, 128), (10, 256)):
                want = index.search_batch_filtered_set(Q, n, ef, s, mo)
                log = {}
                c0 = stats_of(index)
                code, dev = device_call(index, s, Q, n, ef, mo, log_enqueue=log)
                assert code is None
                same(dev, want, "device n=%d ef=%d" % (n, ef))
                assert list(graph_kernels(log).values()) == [1] and len(log) == 1, log  # the enqueue: ONE launch
                d = delta(index, c0)
                assert d["filtered_set_calls"] == 1 and d["filtered_queries_graph"] == 40 and d["mask_set_recounts"] == 0
                assert d["mask_set_words_uploaded"] == 0
                check_rows(index, ridx, Q, n, ef, mask_list, mo, -1, dev, deleted=dele, what="device form")
                code, dev = device_call(index, s, Q, n, ef, mo, optional=False)  # without d_dists and d_counts
                assert code is None and np.array_equal(dev[0], want[0]) and np.array_equal(dev[3], want[3])
            # d_mask_of NULL: every query under row 0
            code, dev = device_call(index, s, Q, 10, 64, None)
            assert code is None
            same(dev, index.search_batch_filtered_set(Q, 10, 64, s), "device, row 0")
        finally:
            if len(dele):
                index.unmark_deleted(dele)
    # limits of the form
    for n, ef in ((65, 65), (10, 257)):
        with pytest.raises(H.HnswError) as e:
            index.search_batch_filtered_device(256, 40, n, ef, s, 0, 256, 0, 0, 256, 0)
        assert e.value.code == _lib.ERR_ARG
    index.set_option("filter_exact_max", 65536)


def test_device_form_refuses_a_row_the_set_does_not_have(glove):
    """the kernel checks d_mask_of, which the host never saw: the query is its own error, no mask word is read"""
    from tests.test_gpu_filtered import masks
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    s = index.mask_set(mask_list)
    Q = queries[:24]
    mo = dealt(24, 6, none_at=(8,)).astype(np.int64)
    index.set_option("filter_exact_max", -1)
    want = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    bad = mo.copy()
    bad[5] = 6            # one past the last row
    bad[17] = 0xFFFFFFFE  # far beyond it (and not HNSW_MASK_NONE)
    c0 = stats_of(index)
    code, dev = device_call(index, s, Q, 10, 64, bad)
    assert code == _lib.ERR_ARG
    for qi in (5, 17):
        assert dev[3][qi].tolist() == [0, 0, 0, _lib.ERR_ARG & 0xFFFFFFFF], dev[3][qi]
        assert dev[2][qi] == 0 and (dev[0][qi] == _lib.UINT32_MAX).all() and np.isinf(dev[1][qi]).all()
    ok = np.ones(24, dtype=bool)
    ok[[5, 17]] = False
    same([x[ok] for x in dev], [x[ok] for x in want], "the other queries")
    assert delta(index, c0)["filtered_set_calls"] == 1
    index.set_option("filter_exact_max", 65536)


# ---- 5. the lists' budget ----------------------------------------------------------------------------------------
def test_cache_budget_zero_compacts_every_call(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(41)
    G = 5
    masks_b = rng.random((G, 1000)) < 0.2
    Q = queries[:30]
    mo = dealt(30, G)
    index.set_option("filter_exact_max", 10 ** 9)
    s = index.mask_set(masks_b)
    kept = index.search_batch_filtered_set(Q, 10, 64, s, mo)
    index.set_option("mask_set_cache_mb", 0)
    try:
        s0 = index.mask_set(masks_b)
        for call in range(3):
            before = stats_of(index, SET_STATS)
            with H.kernel_log() as log:
                got = index.search_batch_filtered_set(Q, 10, 64, s0, mo)
            d = delta(index, before)
            assert d["mask_set_compactions"] == G and log["hx_filt_compact_kernel"] == G, (call, d, dict(log))
            assert d["mask_set_recounts"] == (G if call == 0 else 0)
            same(got, kept, "budget 0, call %d" % call)
    finally:
        index.set_option("mask_set_cache_mb", 64)
        index.set_option("filter_exact_max", 65536)
    check_rows(index, ridx, Q, 10, 64, list(masks_b), mo, 10 ** 9, kept, what="budget")


def test_a_clone_takes_the_cache_budget_from_its_parent():
    """hnsw_clone copies every option: under a parent's "mask_set_cache_mb" = 0 a clone keeps no list and compacts every
    row at every call; a clone of a default parent keeps them (test_cache_budget_zero_compacts_every_call, on one handle)"""
    n_pts, d, G = 600, 16, 2
    vs = rand_vectors(n_pts, d, 23)
    parent = H.HNSW.new(16, 32, d, H.VEC_F32).insert_bulk(vs, 4, False, levels=O.draw_levels(n_pts, 16, 5))
    parent.set_labels(np.arange(n_pts, dtype=np.uint32))
    parent.set_option("filter_exact_max", n_pts + 1)  # every query by the exact path
    masks_b = np.random.default_rng(24).random((G, n_pts)) < 0.3
    Q, mo = rand_vectors(6, d, 25), dealt(6, G)
    got = {}
    for budget in (None, 0):  # the default first
        if budget is not None:
            parent.set_option("mask_set_cache_mb", budget)
        clone = parent.clone()
        s = clone.mask_set(masks_b)
        advance = []
        for call in range(2):
            before = stats_of(clone, SET_STATS)
            got[budget, call] = clone.search_batch_filtered_set(Q, 10, 64, s, mo)
            advance.append(delta(clone, before)["mask_set_compactions"])
        assert (got[budget, 0][4] == 1).all()
        if budget == 0:
            assert advance == [G, G], advance
        else:
            assert advance[1] < G, advance
        s.close()
    for key in got:
        same(got[key], got[None, 0], "clone %s" % (key,))
