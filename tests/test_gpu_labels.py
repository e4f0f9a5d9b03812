"""Label-range filtered search on the MI355X: hnsw_search_batch_filtered_range against hnsw_search_batch_filtered_multi
with masks built from the same predicates (ids, distance bits, counts, stats, paths) and against the CPU restatement
(tests/filtered_restate.py) under `lo <= label[i] <= hi`; what stays in HBM between calls; the device-pointer form
against the host form with filter_exact_max = -1."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import LIMIT, restated
from tests.test_gpu_filtered_multi import NONE, compare_row, glove, graph_kernels, raw_multi  # noqa: F401
from tests.test_gpu_mask_set import delta, same, stats_of, three_paths  # noqa: F401
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
SIX = np.array([3, 77, 4096, 12345, 20000, 29999])
RANGE_STATS = ("label_words_uploaded", "filtered_range_calls", "filtered_range_ranges", "mask_set_words_uploaded", "uploads")
PATH_STATS = ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact")


def as_multi(labels, lo, hi):
    """the ranges of a call as the masks and mask_of of the equivalent _multi call: one mask per distinct (lo, hi)
    pair, [0, UINT32_MAX] as HNSW_MASK_NONE"""
    labels = np.asarray(labels, dtype=np.int64)
    mask_list, row, mo = [], {}, []
    for l, h in zip(lo, hi):
        if (l, h) == (0, MAX):
            mo.append(NONE)
            continue
        if (l, h) not in row:
            row[l, h] = len(mask_list)
            mask_list.append((labels >= l) & (labels <= h))
        mo.append(row[l, h])
    return mask_list, np.array(mo)


def check_range_rows(index, ridx, Q, n, ef, labels, lo, hi, exact_max, got, deleted=(), Qr=None, what="", skip=()):
    """every row against the restatement under `lo <= label[i] <= hi` (and not deleted), as tests/test_gpu_filtered_multi
    check_rows does under a mask; `skip`: rows checked by the caller"""
    Qr = Q if Qr is None else Qr
    lab, dele, cache = [int(x) for x in labels], set(int(i) for i in deleted), {}
    ids, dists, counts, stats, paths = got
    for qi in range(Q.shape[0]):
        if qi in skip:
            continue
        l, h = int(lo[qi]), int(hi[qi])
        allowed = lambda i, l=l, h=h: l <= lab[i] <= h and i not in dele  # noqa: E731
        if (l, h) not in cache:
            cache[l, h] = np.array([i for i in range(len(lab)) if allowed(i)], dtype=np.int64)
        a_ids = cache[l, h]
        w = (what, qi, l, h)
        assert stats[qi, 3] == 0, w
        if a_ids.size <= exact_max:
            assert paths[qi] == 1, w
            want = FR.exact(ridx, Qr[qi], n, a_ids)
        else:
            g = FR.graph(ridx, Qr[qi], n, ef, allowed)
            if g["visited0"] > LIMIT:
                assert paths[qi] == 2, (w, g["visited0"])
            if g["visited0"] + g["maxdeg0"] <= LIMIT:
                assert paths[qi] == 0, (w, g["visited0"])
            want = g if paths[qi] == 0 else FR.exact(ridx, Qr[qi], n, a_ids)
        compare_row(got, qi, want, n, w)


def range_and_multi(index, Q, n, ef, labels, lo, hi, exact_max, what=""):
    """the range call and the _multi call with masks built from the same predicates: equal; -> the range call's result"""
    index.set_option("filter_exact_max", exact_max)
    got = index.search_batch_filtered_range(Q, n, ef, lo, hi)
    mask_list, mo = as_multi(labels, lo, hi)
    same(got, index.search_batch_filtered_multi(Q, n, ef, mask_list, mo), what)
    return got


def raw_range(index, Q, n, ef, lo, hi):
    """the C entry itself -> status and the five arrays (the Python mirror raises on a per-query error)"""
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    lo, hi = np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)
    ids = np.full((nq, n), _lib.UINT32_MAX, dtype=np.uint32)
    dists = np.full((nq, n), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    stats = np.zeros((nq, 4), dtype=np.int32)
    paths = np.zeros(nq, dtype=np.uint8)

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    rc = _lib.lib().hnsw_search_batch_filtered_range(
        index._h, p(Q, C.c_float), nq, n, ef, p(lo, C.c_uint32), p(hi, C.c_uint32), p(ids, C.c_uint32), p(dists, C.c_float),
        p(counts, C.c_uint32), C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)), p(paths, C.c_uint8))
    return rc, (ids, dists, counts, stats.astype(np.int64), paths)


def device_call(index, Q, n, ef, lo, hi, optional=True, log_enqueue=None):
    """the device form with torch tensors in HBM, completed by _finish -> (status or None, the five arrays)"""
    import torch
    dev = torch.device("cuda:0")
    nq = Q.shape[0]

    def u32(a):
        return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    dQ = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    d_lo, d_hi = u32(lo), u32(hi)
    d_ids = torch.zeros((nq, n), dtype=torch.int32, device=dev)
    d_d = torch.zeros((nq, n), dtype=torch.float32, device=dev)
    d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_s = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    args = (dQ, nq, n, ef, d_lo, d_hi, d_ids, d_d if optional else None, d_c if optional else None, d_s, 0)
    torch.cuda.synchronize(dev)
    if log_enqueue is not None:
        with H.kernel_log() as log:
            index.search_batch_filtered_range_device(*args)
        log_enqueue.update(log)
    else:
        index.search_batch_filtered_range_device(*args)
    code = None
    paths = np.zeros(nq, dtype=np.uint8)
    try:
        paths = index.search_batch_filtered_range_device_finish(*args, paths=True)
    except H.HnswError as e:
        code = e.code
    torch.cuda.synchronize(dev)
    return code, (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                  d_s.cpu().numpy().view(np.uint32).astype(np.int64), paths)


# ---- 1, 2. all three paths in one call, f32 and 8-bit; the same under deletions ------------------------------------
def three_path_labels(mask_list):
    """labels by priority over the fixture's masks: 5 on the six ids, 3 on `sparse`, 1 on `dense`, 0 elsewhere"""
    dense, sparse, six = mask_list
    lab = np.zeros(30000, dtype=np.uint32)
    lab[dense] = 1
    lab[sparse] = 3
    lab[six] = 5
    return lab


def three_path_ranges():
    lo = np.tile(np.array([1, 3, 5, 0], dtype=np.uint32), 8)
    hi = np.tile(np.array([1, 3, 5, MAX], dtype=np.uint32), 8)
    return lo, hi


def check_three_paths(index, ridx, Q, lab, lo, hi, got, deleted=(), what=""):
    paths = got[4]
    assert np.array_equal(paths, np.tile(np.array([0, 2, 1, 0], dtype=np.uint8), 8)), paths
    sparse_rows = [qi for qi in range(Q.shape[0]) if lo[qi] == 3]
    check_range_rows(index, ridx, Q, 10, 64, lab, lo, hi, 10, got, deleted=deleted, what=what, skip=sparse_rows)
    # the [3, 3] rows: their walk, restated on the CPU under this label assignment (`sparse` lost nothing it needs to
    # the six ids), fills the largest table -- path 2 is not assumed -- and the rows are the exact restatement's
    labels, dele = [int(x) for x in lab], set(int(i) for i in deleted)
    allowed = lambda i: labels[i] == 3 and i not in dele  # noqa: E731
    a_ids = np.array([i for i in range(30000) if allowed(i)], dtype=np.int64)
    assert 10 < a_ids.size <= 16
    assert FR.graph(ridx, Q[sparse_rows[0]], 10, 64, allowed)["visited0"] > LIMIT
    for qi in sparse_rows:
        assert got[3][qi, 3] == 0
        compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_ids), 10, (what, "sparse", qi))


def test_three_paths_equal_multi_and_the_restatement(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    lab = three_path_labels(mask_list)
    assert (lab[SIX] == 5).all() and int((lab == 5).sum()) == 6
    index.set_labels(lab)
    assert np.array_equal(index.get_labels(), lab)
    lo, hi = three_path_ranges()
    index.search_batch_filtered_range(Q[:1], 10, 64, 0, MAX)  # (uploads the snapshot and the column)
    before = stats_of(index, RANGE_STATS + PATH_STATS)
    got = range_and_multi(index, Q, 10, 64, lab, lo, hi, 10, "three paths")
    d = delta(index, before)  # (the _multi call counts the same queries per path once more)
    assert (d["filtered_queries_graph"], d["filtered_queries_exact"], d["filtered_overflow_exact"]) == (32, 16, 16)
    assert (d["filtered_range_calls"], d["filtered_range_ranges"]) == (1, 4)
    assert d["label_words_uploaded"] == 0 and d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0
    check_three_paths(index, ridx, Q, lab, lo, hi, got, what="three paths")


def test_three_paths_with_deleted_ids(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    lab = three_path_labels(mask_list)
    index.set_labels(lab)
    lo, hi = three_path_ranges()
    rng = np.random.default_rng(84)
    deleted = np.concatenate([rng.choice(30000, 2000, replace=False), [77]])  # one of the six ids among them
    index.mark_deleted(deleted)
    try:
        got = range_and_multi(index, Q, 10, 64, lab, lo, hi, 10, "deleted")
        assert not np.isin(got[0], deleted).any()
        check_three_paths(index, ridx, Q, lab, lo, hi, got, deleted=deleted, what="deleted")
    finally:
        index.unmark_deleted(deleted)


# ---- 6. the device form, on the same index ------------------------------------------------------------------------
def test_device_form_equals_the_host_form(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    lab = three_path_labels(mask_list)
    index.set_labels(lab)
    lo, hi = three_path_ranges()
    lo[[4, 13]], hi[[4, 13]] = 7, 2  # two empty ranges (d_lo > d_hi)
    index.set_option("filter_exact_max", -1)
    try:
        want = index.search_batch_filtered_range(Q, 10, 64, lo, hi)
        assert set(want[4].tolist()) == {0, 2}
        assert (want[2][[4, 13]] == 0).all() and (want[3][[4, 13], 3] == 0).all()
        log = {}
        c0 = stats_of(index, RANGE_STATS + PATH_STATS)
        code, dev = device_call(index, Q, 10, 64, lo, hi, log_enqueue=log)
        assert code is None
        same(dev, want, "device form")
        assert list(graph_kernels(log).values()) == [1] and len(log) == 1, log  # the enqueue: ONE launch
        assert (dev[2][[4, 13]] == 0).all() and (dev[0][[4, 13]] == _lib.UINT32_MAX).all()
        d = delta(index, c0)
        assert d["filtered_range_calls"] == 1 and d["filtered_range_ranges"] == 5 and d["filtered_queries_exact"] == 0
        assert d["filtered_overflow_exact"] == int((want[4] == 2).sum()) > 0
        assert d["filtered_queries_graph"] == 32 - d["filtered_overflow_exact"]
        assert d["label_words_uploaded"] == 0 and d["uploads"] == 0
        code, dev = device_call(index, Q, 10, 64, lo, hi, optional=False)  # without d_dists and d_counts
        assert code is None and np.array_equal(dev[0], want[0]) and np.array_equal(dev[3], want[3])
        assert np.array_equal(dev[4], want[4])
    finally:
        index.set_option("filter_exact_max", 65536)


# ---- 3. the reference's test data: a range per query ------------------------------------------------------------------
def glove_ranges(nq):
    lo = np.array([i % 7 for i in range(nq)], dtype=np.uint32)
    hi = np.array([i % 7 + i % 3 for i in range(nq)], dtype=np.uint32)
    lo[11], hi[11] = 5, 2    # an empty range
    lo[19], hi[19] = 0, MAX  # no filter
    lo[23], hi[23] = 6, MAX  # open above
    lo[30], hi[30] = 7, 9    # in order, and no id has such a label
    return lo, hi


@pytest.mark.parametrize("exact_max", [-1, 50])
def test_reference_test_data_a_range_per_query(glove, exact_max):
    index, ridx, queries = glove
    lab = (np.arange(1000) % 7).astype(np.uint32)
    index.set_labels(lab)
    Q = queries[:40]
    lo, hi = glove_ranges(40)
    n_ranges = len(set(zip(lo.tolist(), hi.tolist())))
    assert n_ranges > 15
    index.search_batch_filtered_range(Q[:1], 10, 64, 0, MAX)  # (uploads the snapshot and the column)
    for n, ef in ((10, 64), (1, 1), (64, 128), (10, 256)):
        before = stats_of(index, RANGE_STATS)
        index.set_option("filter_exact_max", exact_max)
        with H.kernel_log() as log:
            got = index.search_batch_filtered_range(Q, n, ef, lo, hi)
        d = delta(index, before)
        assert (d["filtered_range_calls"], d["filtered_range_ranges"]) == (1, n_ranges)
        assert d["mask_set_words_uploaded"] == 0 and d["label_words_uploaded"] == 0 and d["uploads"] == 0
        # ONE launch of the graph kernel for the graph-path queries, however many distinct ranges
        assert list(graph_kernels(log).values()) == [1], dict(log)
        mask_list, mo = as_multi(lab, lo, hi)
        assert mo[19] == NONE  # [0, UINT32_MAX] is HNSW_MASK_NONE
        same(got, index.search_batch_filtered_multi(Q, n, ef, mask_list, mo), "n=%d ef=%d" % (n, ef))
        check_range_rows(index, ridx, Q, n, ef, lab, lo, hi, exact_max, got, what="glove n=%d ef=%d" % (n, ef))
        for qi in (11, 30):  # the empty range and the range no label lies in: count 0, status OK
            assert got[2][qi] == 0 and got[3][qi, 3] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
        assert np.array_equal(got[4] == 1, (exact_max == 50) & np.isin(np.arange(40), (11, 30)))
    # scalars broadcast: equality with one label for every query
    got = index.search_batch_filtered_range(Q, 10, 64, 3, 3)
    same(got, index.search_batch_filtered_multi(Q, 10, 64, [lab == 3], np.zeros(40, dtype=np.int64)), "broadcast")
    index.set_option("filter_exact_max", 65536)


# ---- 7. ef' above the graph path's limit ---------------------------------------------------------------------------
def test_ef_above_the_graph_paths_limit(glove):
    index, ridx, queries = glove
    index.set_labels((np.arange(1000) % 7).astype(np.uint32))
    Q = queries[:8]
    index.set_option("filter_exact_max", 200)  # one label: 143 ids, exact; two labels: graph
    try:
        got = index.search_batch_filtered_range(Q, 10, 257, 2, 2)  # exact-path ranges only: allowed
        assert (got[4] == 1).all()
        for n, ef in ((10, 257), (1, 1000)):
            with pytest.raises(H.HnswError) as e:
                index.search_batch_filtered_range(Q, n, ef, [2, 2, 2, 2, 2, 2, 2, 1], [2, 2, 2, 2, 2, 2, 2, 2])
            assert e.value.code == _lib.ERR_ARG, (n, ef)
    finally:
        index.set_option("filter_exact_max", 65536)


# ---- 4. residency ----------------------------------------------------------------------------------------------------
def test_residency_and_labels_of_later_inserts():
    d, n0 = 24, 1500
    vs = rand_vectors(n0, d, 61)
    index = H.HNSW.new(8, 32, d, H.VEC_QUANT8).insert_bulk(vs, 2, False, levels=O.draw_levels(n0, 8, 3))
    index.search_batch(vs[:2], 10, 32)  # (uploads the snapshot)
    lab = (np.arange(n0) % 5).astype(np.uint32)
    index.set_labels(lab)
    qs = rand_vectors(12, d, 63)
    lo = np.array([i % 5 for i in range(12)], dtype=np.uint32)
    hi = np.minimum(lo + np.arange(12) % 2, 4).astype(np.uint32)
    index.set_option("filter_exact_max", -1)
    # the first search uploads the column: one whole copy, two labels per word
    before = stats_of(index, RANGE_STATS)
    with H.kernel_log() as log:
        first = index.search_batch_filtered_range(qs, 10, 32, lo, hi)
    d_ = delta(index, before)
    assert d_["label_words_uploaded"] == n0 // 2 and d_["uploads"] == 0 and d_["mask_set_words_uploaded"] == 0
    assert "hx_deleted_scatter_kernel" not in log and list(graph_kernels(log).values()) == [1], dict(log)
    mask_list, mo = as_multi(lab, lo, hi)
    same(first, index.search_batch_filtered_multi(qs, 10, 32, mask_list, mo), "first call")
    # the identical second search uploads nothing
    before = stats_of(index, RANGE_STATS)
    with H.kernel_log() as log:
        second = index.search_batch_filtered_range(qs, 10, 32, lo, hi)
    assert delta(index, before)["label_words_uploaded"] == 0 and "hx_deleted_scatter_kernel" not in log
    same(second, first, "second call")
    # labels of ids in w = 3 words change (3 < 750 / 8): exactly those words travel, by one scatter, no snapshot upload
    ids = np.array([10, 11, 500, 1001])  # words 5, 250, 500
    lab[ids] = [4, 3, 2, 2]
    assert (index.get_labels(ids) != lab[ids]).all()
    index.set_labels(lab[ids], ids)
    index.set_labels(lab[ids], ids)  # (idempotent: nothing more is listed)
    before = stats_of(index, RANGE_STATS)
    with H.kernel_log() as log:
        third = index.search_batch_filtered_range(qs, 10, 32, lo, hi)
    d_ = delta(index, before)
    assert d_["label_words_uploaded"] == 3 and d_["uploads"] == 0 and log["hx_deleted_scatter_kernel"] == 1, (d_, dict(log))
    mask_list, mo = as_multi(lab, lo, hi)
    same(third, index.search_batch_filtered_multi(qs, 10, 32, mask_list, mo), "after set_labels")
    # insert_vec: the new id has label 0 without a call and is found under [0, 0] ...
    new = rand_vectors(1, d, 62)[0]
    assert index.insert_vec(new, level=0) == n0
    assert index.get_labels([n0]).tolist() == [0]
    lab = np.concatenate([lab, [0]]).astype(np.uint32)
    for exact_max in (-1, 10 ** 9):
        index.set_option("filter_exact_max", exact_max)
        before = stats_of(index, RANGE_STATS)
        got = index.search_batch_filtered_range(new[None, :], 10, 32, 0, 0)
        assert delta(index, before)["label_words_uploaded"] == 0  # (the copy was made with room: its zeros serve)
        assert n0 in got[0][0], (exact_max, got[0][0])
        same(got, index.search_batch_filtered_multi(new[None, :], 10, 32, [lab == 0], [0]), "new id under [0, 0]")
        assert n0 not in index.search_batch_filtered_range(new[None, :], 10, 32, 1, 4)[0][0]
    # ... and, after set_labels, under its new label
    index.set_labels([9], [n0])
    lab[n0] = 9
    for exact_max in (-1, 10 ** 9):
        index.set_option("filter_exact_max", exact_max)
        before = stats_of(index, RANGE_STATS)
        got = index.search_batch_filtered_range(new[None, :], 10, 32, 9, 9)
        assert delta(index, before)["label_words_uploaded"] == (1 if exact_max == -1 else 0)
        assert got[2][0] == 1 and got[0][0, 0] == n0, got[0][0]
        assert n0 not in index.search_batch_filtered_range(new[None, :], 10, 32, 0, 0)[0][0]
    assert index.stat("point_patches") == 1 and index.stat("patch_fallbacks") == 0


# ---- 5. a NaN query; the cosine option ------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_max", [-1, 200])
def test_a_nan_query_is_its_own_error(glove, exact_max):
    index, ridx, queries = glove
    lab = (np.arange(1000) % 7).astype(np.uint32)
    index.set_labels(lab)
    Q = queries[:24].copy()
    lo = np.array([i % 7 for i in range(24)], dtype=np.uint32)
    hi = (lo + np.arange(24) % 2).astype(np.uint32)
    Q[9, 4] = np.nan   # one label (143 ids): the graph path under -1, the exact path under 200
    Q[20, 0] = np.nan  # two labels: the graph path under both
    lo[9], hi[9] = 2, 2
    lo[20], hi[20] = 3, 4
    index.set_option("filter_exact_max", exact_max)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_range(Q, 10, 64, lo, hi)
    assert e.value.code == _lib.ERR_NAN_INPUT
    rc, got = raw_range(index, Q, 10, 64, lo, hi)
    mask_list, mo = as_multi(lab, lo, hi)
    rc_m, want = raw_multi(index, Q, 10, 64, mask_list, mo)
    assert rc == rc_m == _lib.ERR_NAN_INPUT
    same(got, want, "nan")
    assert got[4][9] == (1 if exact_max == 200 else 0)
    for qi in (9, 20):
        assert got[3][qi, 3] == _lib.ERR_NAN_INPUT and got[2][qi] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
    check_range_rows(index, ridx, Q, 10, 64, lab, lo, hi, exact_max, got, what="nan", skip=(9, 20))
    if exact_max == -1:  # the device form reports the same rows and the same first error
        code, dev = device_call(index, Q, 10, 64, lo, hi)
        assert code == _lib.ERR_NAN_INPUT
        same(dev[:4], (got[0], got[1], got[2], got[3].view(np.uint64).astype(np.uint32).astype(np.int64)), "device nan")
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
    index.set_labels(lab)
    lo = np.array([i % 5 for i in range(20)], dtype=np.uint32)
    hi = (lo + np.array([0, 5, 14] * 7)[:20]).astype(np.uint32)  # about 100, 600 and 1500 ids
    for exact_max in (-1, 300):
        got = range_and_multi(index, qs, 10, 64, lab, lo, hi, exact_max, "cosine %d" % exact_max)
        check_range_rows(index, ridx, qs, 10, 64, lab, lo, hi, exact_max, got, what="cosine", Qr=unit(qs))
        assert (got[4] == 1).any() == (exact_max == 300)
    index.set_option("filter_exact_max", -1)
    want = index.search_batch_filtered_range(qs, 10, 64, lo, hi)
    code, dev = device_call(index, qs, 10, 64, lo, hi)
    assert code is None
    same(dev, want, "device form, cosine")
