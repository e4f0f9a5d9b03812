"""Label-set filtered search on the MI355X: hnsw_search_batch_filtered_ranges -- several label ranges per query, an id
allowed when its label lies in any of them -- against hnsw_search_batch_filtered_multi with the unions materialised as
masks (ids, distance bits, counts, stats, paths) and against the CPU restatement (tests/filtered_restate.py) under the
union; n_ranges == 1 against hnsw_search_batch_filtered_range, launch for launch; canonical forms; every compiled form of
the graph kernel; launches and uploads; the device-pointer form against the host form with filter_exact_max = -1."""

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import LIMIT
from tests.test_gpu_filtered_multi import (FORMS, NONE, check_rows, compare_row, glove, graph_kernels,  # noqa: F401
                                           predicates)
from tests.test_gpu_labels import glove_ranges, three_path_labels
from tests.test_gpu_mask_set import delta, same, stats_of, three_paths  # noqa: F401
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
STATS = ("filtered_ranges_calls", "filtered_ranges_groups", "filtered_range_calls", "label_words_uploaded",
         "mask_set_words_uploaded", "uploads")
PATH_STATS = ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact")


def union(labels, members):
    """the ids whose label lies in at least one member ((lo, hi) or an int x: [x, x]; lo > hi: none)"""
    labels = np.asarray(labels, dtype=np.int64)
    m = np.zeros(labels.shape[0], dtype=bool)
    for x in members:
        l, h = (x, x) if isinstance(x, (int, np.integer)) else x
        m |= (labels >= l) & (labels <= h)
    return m


def as_multi(labels, lists):
    """the range lists of a call as the masks and mask_of of the equivalent _multi call: one mask per distinct union,
    the union that is every label as HNSW_MASK_NONE"""
    mask_list, row, mo = [], {}, []
    for r in lists:
        m = union(labels, r)
        covered = np.zeros(1, dtype=bool)
        if m.all():  # every id: but is it every LABEL?  (the planner's "no filter" is [0, UINT32_MAX])
            covered = union(np.array([0, 1, MAX - 1, MAX, 12345678]), r)
        if covered.all():
            mo.append(NONE)
            continue
        key = m.tobytes()
        if key not in row:
            row[key] = len(mask_list)
            mask_list.append(m)
        mo.append(row[key])
    return mask_list, np.array(mo)


def ranges_and_multi(index, Q, n, ef, labels, lists, exact_max, what=""):
    """the ranges call and the _multi call with the unions as masks: equal -> the ranges call's result, masks, mask_of"""
    index.set_option("filter_exact_max", exact_max)
    got = index.search_batch_filtered_ranges(Q, n, ef, lists)
    mask_list, mo = as_multi(labels, lists)
    same(got, index.search_batch_filtered_multi(Q, n, ef, mask_list, mo), what)
    return got, mask_list, mo


def device_call(index, Q, n, ef, lists, optional=True, log_enqueue=None):
    """the device form with torch tensors in HBM, completed by _finish -> (status or None, the five arrays)"""
    import torch
    dev = torch.device("cuda:0")
    nq = Q.shape[0]
    lo, hi = H.pack_ranges(lists, nq)

    def u32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    dQ = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    d_lo, d_hi = u32(lo), u32(hi)
    d_ids = torch.zeros((nq, n), dtype=torch.int32, device=dev)
    d_d = torch.zeros((nq, n), dtype=torch.float32, device=dev)
    d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_s = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    args = (dQ, nq, n, ef, lo.shape[1], d_lo, d_hi, d_ids, d_d if optional else None, d_c if optional else None, d_s, 0)
    torch.cuda.synchronize(dev)
    if log_enqueue is not None:
        with H.kernel_log() as log:
            index.search_batch_filtered_ranges_device(*args)
        log_enqueue.update(log)
    else:
        index.search_batch_filtered_ranges_device(*args)
    code = None
    paths = np.zeros(nq, dtype=np.uint8)
    try:
        paths = index.search_batch_filtered_ranges_device_finish(*args, paths=True)
    except H.HnswError as e:
        code = e.code
    torch.cuda.synchronize(dev)
    return code, (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                  d_s.cpu().numpy().view(np.uint32).astype(np.int64), paths)


# ---- 1. all three paths in one call, f32 and 8-bit; the same under deletions ------------------------------------------
# labels (three_path_labels): 1 on `dense`, 3 on `sparse` (16 ids), 5 on the six ids, 0 elsewhere.  The lists, by kind:
KINDS = (
    [1],                    # dense: the graph path ends early (0)
    [(3, 3), (1, 0)],       # sparse: the walk fills the largest table (2)
    [(7, 2), 5],            # the six ids: exact (1)
    [5, 1],                 # dense or six, unsorted: 0
    [(1, 0), (7, 2)],       # all members empty: count 0, status OK (exact: A = 0)
    [(0, 2), (3, MAX)],     # adjacent members that merge into [0, UINT32_MAX]: no filter
    [5, 3],                 # sparse or six, two disjoint members: 22 ids, the exact path under a LIST when it gets there
)


def run_three_paths(index, ridx, mask_list, Q, deleted=(), what=""):
    lab = three_path_labels(mask_list)
    index.set_labels(lab)
    lists = [KINDS[i % len(KINDS)] for i in range(Q.shape[0])]
    kind_of = np.arange(Q.shape[0]) % len(KINDS)
    try:
        index.search_batch_filtered_ranges(Q[:1], 10, 64, [[(0, MAX)]])  # (uploads the snapshot and the column)
        before = stats_of(index, STATS + PATH_STATS)
        got, masks, mo = ranges_and_multi(index, Q, 10, 64, lab, lists, 10, what)
        d = delta(index, before)
        paths = got[4]
        assert (paths[kind_of == 0] == 0).all() and (paths[kind_of == 3] == 0).all() and (paths[kind_of == 5] == 0).all()
        assert (paths[kind_of == 1] == 2).all() and (paths[kind_of == 2] == 1).all() and (paths[kind_of == 4] == 1).all()
        assert (d["filtered_ranges_calls"], d["filtered_ranges_groups"], d["filtered_range_calls"]) == (1, len(KINDS), 0)
        assert d["label_words_uploaded"] == 0 and d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0
        # (the _multi call counts the same queries per path once more)
        assert d["filtered_queries_graph"] == 2 * int((paths == 0).sum())
        assert d["filtered_queries_exact"] == 2 * int((paths == 1).sum())
        assert d["filtered_overflow_exact"] == 2 * int((paths == 2).sum())
        assert mo[5] == NONE and (got[2][kind_of == 4] == 0).all() and (got[3][:, 3] == 0).all()
        assert (got[0][kind_of == 4] == _lib.UINT32_MAX).all()
        # the rows against the restatement under the union; those whose walk fills the largest table (path 2 is not
        # assumed: the walk is restated on the CPU) against the exact restatement
        pred = predicates(index, masks, deleted)
        over = [qi for qi in range(Q.shape[0]) if kind_of[qi] in (1, 6)]
        check_rows(index, ridx, Q, 10, 64, masks, mo, 10, got, deleted=deleted, what=what, skip=over)
        for k in (1, 6):
            qs = [qi for qi in over if kind_of[qi] == k]
            allowed, a_ids = pred(int(mo[qs[0]]))
            assert 10 < a_ids.size <= 22
            assert FR.graph(ridx, Q[qs[0]], 10, 64, allowed)["visited0"] > LIMIT
            assert (paths[qs] == 2).all(), paths
            for qi in qs:
                compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_ids), 10, (what, "overflow", qi))
        if len(deleted):
            assert not np.isin(got[0], deleted).any()
    finally:
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


# ---- 2. n_ranges == 1 is hnsw_search_batch_filtered_range ------------------------------------------------------------
@pytest.mark.parametrize("exact_max", [-1, 50])
def test_one_range_per_query_equals_the_range_call(glove, exact_max):
    index, ridx, queries = glove
    index.set_labels((np.arange(1000) % 7).astype(np.uint32))
    Q = queries[:40]
    lo, hi = glove_ranges(40)  # with an empty range, [0, MAX], and a range no label lies in
    lists = [[(int(l), int(h))] for l, h in zip(lo, hi)]
    index.set_option("filter_exact_max", exact_max)
    try:
        index.search_batch_filtered_range(Q[:1], 10, 64, 0, MAX)  # (uploads the snapshot and the column)
        for n, ef in ((10, 64), (64, 128)):
            with H.kernel_log() as log_r:
                want = index.search_batch_filtered_range(Q, n, ef, lo, hi)
            before = stats_of(index, STATS)
            with H.kernel_log() as log:
                got = index.search_batch_filtered_ranges(Q, n, ef, lists)
            same(got, want, "n=%d ef=%d" % (n, ef))
            assert dict(log) == dict(log_r), (dict(log), dict(log_r))  # the same kernels, the same number of times
            d = delta(index, before)
            assert (d["filtered_ranges_calls"], d["filtered_range_calls"]) == (1, 0)
            assert d["filtered_ranges_groups"] == len(set(zip(lo.tolist(), hi.tolist())))
    finally:
        index.set_option("filter_exact_max", 65536)


# ---- 3. canonical forms ----------------------------------------------------------------------------------------------
def edge_labels():
    rng = np.random.default_rng(31)
    lab = rng.integers(0, 41, size=1000).astype(np.uint32)
    lab[[0, 17, 500]] = MAX
    lab[[1, 18, 999]] = MAX - 1
    lab[[2, 19]] = 0
    return lab


@pytest.mark.parametrize("exact_max", [-1, 10 ** 9])
def test_lists_with_one_canonical_form_are_one_group(glove, exact_max):
    index, ridx, queries = glove
    lab = edge_labels()
    index.set_labels(lab)
    alike = [[(1, 2), (3, 4)], [(3, 4), (1, 2)], [(1, 4)], [(1, 3), (2, 4)], [1, 2, 3, 4], [(1, 4), (5, 2)],
             [(2, 2), (1, 1), (4, 4), (3, 3), (1, 1), (9, 0)], [(1, 4), (1, 4), (2, 3)]]
    Q = np.repeat(queries[:1], len(alike), axis=0)
    index.set_option("filter_exact_max", exact_max)
    try:
        index.search_batch_filtered_ranges(Q[:1], 10, 64, [[0]])
        before = stats_of(index, STATS)
        with H.kernel_log() as log:
            got = index.search_batch_filtered_ranges(Q, 10, 64, alike)
        d = delta(index, before)
        assert (d["filtered_ranges_calls"], d["filtered_ranges_groups"]) == (1, 1)
        if exact_max > 0:  # one group: one compaction, one scan, one merge
            assert log["hx_filt_compact_kernel"] == 1 and log["hx_filt_merge_kernel"] == 1 and not graph_kernels(log)
        for a in got[:4]:
            assert (a == a[0]).all()
        want = index.search_batch_filtered_multi(Q, 10, 64, [(lab >= 1) & (lab <= 4)], np.zeros(len(alike), dtype=np.int64))
        same(got, want, "alike")
        assert got[2][0] == 10
    finally:
        index.set_option("filter_exact_max", 65536)


@pytest.mark.parametrize("exact_max", [-1, 10 ** 9])
def test_sixteen_singletons_and_the_top_of_the_label_space(glove, exact_max):
    index, ridx, queries = glove
    lab = edge_labels()
    index.set_labels(lab)
    Q = queries[:12]
    sixteen = [2 * j for j in range(16)]
    lists = [sixteen, sixteen[::-1], [(MAX, MAX), (MAX - 1, MAX - 1)], [(MAX - 1, MAX - 1), (MAX, MAX), (0, 0)],
             [(0, 5), (MAX, MAX)],      # MAX + 1 must not wrap to 0: these do not touch
             [(MAX, MAX), (0, 0)], [(6, MAX), (0, 4)], [(MAX - 1, MAX), (40, MAX - 2)],
             [(1, MAX), (0, 0)],        # touches at 0 / 1: no filter
             [MAX], [(MAX, MAX - 1), MAX - 1], list(range(25, 41))]
    got, masks, mo = ranges_and_multi(index, Q, 10, 64, lab, lists, exact_max, "edges")
    try:
        assert mo[0] == mo[1] and mo[8] == NONE and (mo[[4, 5, 6]] != NONE).all()
        assert got[2][2] == 6 and got[2][9] == 3 and got[2][10] == 3  # three ids labelled MAX, three MAX - 1
        assert set(got[0][9][:3].tolist()) == {0, 17, 500} and set(got[0][10][:3].tolist()) == {1, 18, 999}
        check_rows(index, ridx, Q, 10, 64, masks, mo, exact_max, got, what="edges")
        for qi, r in enumerate(lists):
            assert index.count_labels_in_ranges(r) == int(union(lab, r).sum()), r
    finally:
        index.set_option("filter_exact_max", 65536)


# ---- 4. every compiled form of the graph kernel reads its list ------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(H.VEC_F32, 100), (H.VEC_F32, 128), (H.VEC_F32, 37), (H.VEC_QUANT8, 100),
                                    (H.VEC_QUANT8, 37)])
def test_shapes(kind, d):
    vs = rand_vectors(3000, d, 40 + d)
    qs = rand_vectors(30, d, 41 + d)
    index = H.HNSW.new(16, 64, d, kind).insert_bulk(vs, 4, False, levels=O.draw_levels(3000, 16, 2))
    index.set_option("filter_exact_max", -1)
    rng = np.random.default_rng(50 + d)
    lab = rng.integers(0, 10, size=3000).astype(np.uint32)
    index.set_labels(lab)
    # K = 3 with one empty member, at every position; a list that is all empty; one whose only member is the last
    shapes = [[(4, 1), 2, (5, 6)], [0, (9, 3), 9], [(7, 8), 1, (1, 0)], [(1, 0), (2, 1), (3, 2)], [(1, 0), (1, 0), 4],
              [(0, 3), (2, 5), (7, 2)], [9, 9, (1, 0)]]
    lists = [shapes[i % len(shapes)] for i in range(30)]
    masks, mo = as_multi(lab, lists)
    index.search_batch_filtered_ranges(qs[:2], 10, 64, lists[:2])  # (uploads the snapshot and the column)
    for (n, ef), r in (((10, 64), 1), ((64, 128), 2), ((64, 256), 4)):
        with H.kernel_log() as log:
            got = index.search_batch_filtered_ranges(qs, n, ef, lists)
        assert set(graph_kernels(log)) == {"hx_filt_graph_kernel<%s, %d>" % (FORMS[kind, d], r)}, dict(log)
        assert list(graph_kernels(log).values()) == [1] and "hx_filt_compact_kernel" not in log, dict(log)
        assert (got[4] == 0).all()
        same(got, index.search_batch_filtered_multi(qs, n, ef, masks, mo), "d=%d n=%d ef=%d" % (d, n, ef))
        assert got[2][3] == 0 and got[3][3, 3] == 0 and (got[0][3] == _lib.UINT32_MAX).all()  # all members empty
        assert got[2][4] > 0 and (lab[got[0][4][: got[2][4]]] == 4).all()  # the only member that is not empty is the last


# ---- 5. launches and uploads ---------------------------------------------------------------------------------------------
def test_one_graph_launch_and_nothing_uploaded(glove):
    index, ridx, queries = glove
    lab = (np.arange(1000) % 40).astype(np.uint32)
    index.set_labels(lab)
    Q = queries[:16]
    four = [[3, 7, 12], [(0, 9), (20, 29)], [(30, 39), 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [39, 0]]
    lists = [four[i % 4] for i in range(16)]
    index.set_option("filter_exact_max", -1)
    try:
        index.search_batch_filtered_ranges(Q[:1], 10, 64, [[0]])  # (uploads the snapshot and the column)
        before = stats_of(index, STATS)
        with H.kernel_log() as log:
            got = index.search_batch_filtered_ranges(Q, 10, 64, lists)
        d = delta(index, before)
        assert list(graph_kernels(log).values()) == [1], dict(log)  # ONE launch for the four lists
        assert "hx_filt_compact_kernel" not in log and "hx_deleted_scatter_kernel" not in log, dict(log)
        assert (d["filtered_ranges_calls"], d["filtered_ranges_groups"]) == (1, 4)
        assert d["mask_set_words_uploaded"] == 0 and d["uploads"] == 0 and d["label_words_uploaded"] == 0
        masks, mo = as_multi(lab, lists)
        same(got, index.search_batch_filtered_multi(Q, 10, 64, masks, mo), "four lists")
        # a label changes: its word travels with the next call, and with that call alone
        lab[123] = 7
        index.set_labels([7], [123])
        before = stats_of(index, STATS)
        got = index.search_batch_filtered_ranges(Q, 10, 64, lists)
        d = delta(index, before)
        assert d["label_words_uploaded"] == 1 and d["uploads"] == 0 and d["mask_set_words_uploaded"] == 0
        masks, mo = as_multi(lab, lists)
        same(got, index.search_batch_filtered_multi(Q, 10, 64, masks, mo), "after set_labels")
        before = stats_of(index, STATS)
        index.search_batch_filtered_ranges(Q, 10, 64, lists)
        assert delta(index, before)["label_words_uploaded"] == 0
    finally:
        index.set_option("filter_exact_max", 65536)


# ---- 6. the device form, on the three-path index ---------------------------------------------------------------------------
def test_device_form_equals_the_host_form(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    lab = three_path_labels(mask_list)
    index.set_labels(lab)
    lists = [KINDS[i % len(KINDS)] for i in range(Q.shape[0])]
    index.set_option("filter_exact_max", -1)
    try:
        want = index.search_batch_filtered_ranges(Q, 10, 64, lists)
        assert set(want[4].tolist()) == {0, 2}  # path-2 queries included
        empty = [qi for qi in range(Q.shape[0]) if qi % len(KINDS) == 4]
        assert (want[2][empty] == 0).all() and (want[3][empty, 3] == 0).all()
        log = {}
        c0 = stats_of(index, STATS + PATH_STATS)
        code, dev = device_call(index, Q, 10, 64, lists, log_enqueue=log)
        assert code is None
        same(dev, want, "device form")
        assert list(graph_kernels(log).values()) == [1] and len(log) == 1, log  # the enqueue: ONE launch
        assert (dev[2][empty] == 0).all() and (dev[0][empty] == _lib.UINT32_MAX).all()
        d = delta(index, c0)
        assert (d["filtered_ranges_calls"], d["filtered_ranges_groups"], d["filtered_range_calls"]) == (1, len(KINDS), 0)
        assert d["filtered_queries_exact"] == 0
        assert d["filtered_overflow_exact"] == int((want[4] == 2).sum()) > 0
        assert d["filtered_queries_graph"] == Q.shape[0] - d["filtered_overflow_exact"]
        assert d["label_words_uploaded"] == 0 and d["uploads"] == 0
        code, dev = device_call(index, Q, 10, 64, lists, optional=False)  # without d_dists and d_counts
        assert code is None and np.array_equal(dev[0], want[0]) and np.array_equal(dev[3], want[3])
        assert np.array_equal(dev[4], want[4])
    finally:
        index.set_option("filter_exact_max", 65536)


def test_the_counters_advance_at_finish(glove):
    import torch
    index, ridx, queries = glove
    index.set_labels((np.arange(1000) % 40).astype(np.uint32))
    Q = queries[:8]
    lists = [[i, (20, 20 + i)] for i in range(8)]
    dev = torch.device("cuda:0")
    lo, hi = H.pack_ranges(lists, 8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    dQ, d_lo, d_hi = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev), t(lo), t(hi)
    d_ids = torch.zeros((8, 10), dtype=torch.int32, device=dev)
    d_s = torch.zeros((8, 4), dtype=torch.int32, device=dev)
    args = (dQ, 8, 10, 64, 2, d_lo, d_hi, d_ids, None, None, d_s, 0)
    index.search_batch_filtered_ranges(Q[:1], 10, 64, [[0]])  # (uploads the snapshot and the column)
    before = stats_of(index, STATS + PATH_STATS)
    index.search_batch_filtered_ranges_device(*args)
    assert all(v == 0 for v in delta(index, before).values())
    index.search_batch_filtered_ranges_device_finish(*args)
    d = delta(index, before)
    assert (d["filtered_ranges_calls"], d["filtered_ranges_groups"], d["filtered_queries_graph"]) == (1, 8, 8)
    index.set_option("filter_exact_max", -1)
    try:
        want = index.search_batch_filtered_ranges(Q, 10, 64, lists)
    finally:
        index.set_option("filter_exact_max", 65536)
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), want[0])


# ---- 7. the reference's test data: a list per query ----------------------------------------------------------------------
def glove_lists(nq):
    """over labels 0..39 (25 ids each): one, two (50 ids: exact under 50) and three labels, ranges, ragged lengths"""
    shapes = [[3], [3, 7], [3, 7, 12], [(0, 1), (4, 5), 39], [(10, 19)], [(10, 12), (11, 19), 15], [(5, 2)], [],
              [(0, MAX)], [(0, 19), (20, MAX)], [38, 39, (40, 50)], [(41, MAX)], list(range(0, 32, 2)), [(7, 2), 8, 9]]
    return [shapes[i % len(shapes)] for i in range(nq)]


@pytest.mark.parametrize("exact_max", [-1, 50])
@pytest.mark.parametrize("n,ef", [(10, 64), (1, 1), (64, 100), (64, 10)])
def test_reference_test_data_a_list_per_query(glove, n, ef, exact_max):
    index, ridx, queries = glove
    lab = (np.arange(1000) % 40).astype(np.uint32)
    index.set_labels(lab)
    Q = queries[:28]
    lists = glove_lists(28)
    try:
        index.search_batch_filtered_ranges(Q[:1], 10, 64, [[0]])  # (uploads the snapshot and the column)
        got, masks, mo = ranges_and_multi(index, Q, n, ef, lab, lists, exact_max, "glove n=%d ef=%d" % (n, ef))
        check_rows(index, ridx, Q, n, ef, masks, mo, exact_max, got, what="glove n=%d ef=%d" % (n, ef))
        assert mo[8] == NONE and mo[9] == NONE
        for qi in (6, 7, 11):  # all members empty, no member, and a range no label lies in: count 0, status OK
            assert got[2][qi] == 0 and got[3][qi, 3] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
        if exact_max == 50:  # exact: the empty unions, one label (25 ids) and two (50 ids: a list of two, or one range)
            assert np.array_equal(np.flatnonzero(got[4][:14] == 1), [0, 1, 6, 7, 10, 11, 13])
        else:
            assert (got[4] == 0).all()
    finally:
        index.set_option("filter_exact_max", 65536)
