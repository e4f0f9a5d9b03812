"""Filtered search and deletion over f16-resident rows (option "rows_f16", search_filtered16.hip)
against the CPU restatement (tests/filtered_restate.py) over the widened rows X16 = X.astype(float16).astype(float32) on
the product's own graph: ids, distance bits, counts, the three counters and the path of every query are equal, and the
launch log names the hx_filt16 instantiation that ran.  Every parity case fails on a library that refuses these calls."""
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from oracle import restate_np as R
from tests import filtered_restate as FR
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu


def widen(X):
    return X.astype(np.float16).astype(np.float32)


def restated(index, X):
    layers = [index.get_layer(l).csr() for l in range(index.nb_layers())]
    return R.Index.from_csr(widen(X), index.vec_kind, layers, int(index.params.ep))


def f16_index(X, m):
    index = H.HNSW.new(m, 32, X.shape[1], H.VEC_F32)
    index.set_option("rows_f16", 1)
    return index.insert_bulk(X, 4, False, levels=O.draw_levels(len(X), m, 3))


def build(n, d, m, nq):
    X, Q = rand_vectors(n, d, 300 + d) * 2 - 0.5, rand_vectors(nq, d, 400 + d) * 2 - 0.5
    index = f16_index(X, m)
    return index, X, Q, restated(index, X)


def graph_kernel(d, ef):
    return "hx_filt16_graph_kernel<%d, %d>" % (d if d in (128, 256, 768) else 0, 1 if ef <= 64 else 2 if ef <= 128 else 4)


def scan_kernel(d):
    return "hx_filt16_scan_kernel<%d>" % (d if d in (128, 256, 768) else 0)


def check(index, ridx, Q, n, ef, allowed, call, exact=False, what=""):
    """call() -> (ids, dists, counts, stats, paths) of the product; allowed: one bool row over the ids per query"""
    index.set_option("filter_exact_max", 1 << 30 if exact else -1)
    d = Q.shape[1]
    with H.kernel_log() as log:
        ids, dists, counts, stats, paths = call()
    assert (scan_kernel(d) if exact else graph_kernel(d, max(ef, n))) in log, (what, dict(log))
    assert not any(k.startswith(("hx_filt_graph", "hx_filt_scan")) for k in log), dict(log)
    assert (stats[:, 3] == 0).all() and (np.asarray(paths) == (1 if exact else 0)).all(), (what, paths)
    for qi in range(len(Q)):
        a = np.broadcast_to(allowed, (len(Q), len(allowed[-1])))[qi]
        want = FR.exact(ridx, Q[qi], n, np.flatnonzero(a)) if exact else FR.graph(ridx, Q[qi], n, ef, lambda i: bool(a[i]))
        w_ids, w_d, w_c = FR.padded(want, n)
        assert counts[qi] == w_c and np.array_equal(ids[qi], w_ids), (what, qi, ids[qi], w_ids)
        assert np.array_equal(dists[qi].view(np.uint32), w_d.view(np.uint32)), (what, qi)
        assert tuple(int(x) for x in stats[qi, :3]) == tuple(want["counters"]), (what, qi, stats[qi], want["counters"])


def two_rows(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01])


@pytest.mark.parametrize("d", [1, 7, 9, 100, 136, 128, 256, 768])
def test_row_forms(d):
    """the lane-per-row form on both sides of the 8-element piece and just off a line, and the three gathers"""
    index, X, Q, ridx = build(600, d, 8, 12)
    rows, mo = two_rows(600), np.arange(12) % 2
    ms = index.mask_set(rows)
    for ef in (1, 17, 64):
        check(index, ridx, Q, 10, ef, rows[mo], lambda: index.search_batch_filtered_set(Q, 10, ef, ms, mo), what="ef=%d" % ef)


@pytest.mark.parametrize("d", [24, 128])
@pytest.mark.parametrize("ef", [100, 256])
def test_list_widths(d, ef):
    index, X, Q, ridx = build(600, d, 8, 8)
    rows, mo = two_rows(600), np.arange(8) % 2
    check(index, ridx, Q, 64, ef, rows[mo], lambda: index.search_batch_filtered_multi(Q, 64, ef, rows, mo))


@pytest.mark.parametrize("d", [128, 256])
def test_more_than_32_wanted_rows_in_a_pass(d):
    index, X, Q, ridx = build(3000, d, 32, 12)  # S0 = 64: the four-lanes-per-row round in the walk
    rows, mo = two_rows(3000)[:1], np.zeros(12, dtype=np.int64)
    check(index, ridx, Q, 10, 64, rows[mo], lambda: index.search_batch_filtered_multi(Q, 10, 64, rows, mo))


@functools.lru_cache(maxsize=None)
def big(d):
    """3000 rows with labels 0 .. 9, 30 queries: built once per dimension"""
    index, X, Q, ridx = build(3000, d, 8, 30)
    labels = np.random.default_rng(3).integers(0, 10, 3000).astype(np.uint32)
    index.set_labels(labels)
    return index, Q, ridx, labels


def test_every_filter_form():
    index, Q, ridx, lab = big(128)
    Q, n, ef = Q[:10], 10, 64
    rows = two_rows(3000)
    ms = index.mask_set(rows)
    in_range = (lab >= 2) & (lab <= 5)
    check(index, ridx, Q, n, ef, in_range[None], lambda: index.search_batch_filtered_range(Q, n, ef, 2, 5), what="range")
    mo = np.array([0, -1] * 5)
    both = np.where((mo >= 0)[:, None], rows[0][None] & in_range[None], in_range[None])
    check(index, ridx, Q, n, ef, both, lambda: index.search_batch_filtered_set_range(Q, n, ef, ms, mo, 2, 5), what="range AND row")
    three = [[(1, 0), (7, 8), 3]] * 10  # K = 3, the first member empty
    check(index, ridx, Q, n, ef, (((lab >= 7) & (lab <= 8)) | (lab == 3))[None],
          lambda: index.search_batch_filtered_ranges(Q, n, ef, three), what="three ranges")
    none = np.where((mo >= 0)[:, None], rows[1][None], np.ones((1, 3000), dtype=bool))
    check(index, ridx, Q, n, ef, none, lambda: index.search_batch_filtered_multi(Q, n, ef, rows, np.where(mo >= 0, 1, -1)), what="none")
    check(index, ridx, Q, n, ef, np.zeros((1, 3000), dtype=bool), lambda: index.search_batch_filtered_range(Q, n, ef, 5, 2), what="empty")
    ids, dists, count, path = index.search_filtered(Q[0], n, ef, 2, 5, ms, 0)  # the one-query entry: the same walk
    want = FR.padded(FR.graph(ridx, Q[0], n, ef, lambda i: bool(both[0][i])), n)
    assert count == want[2] and np.array_equal(ids, want[0]) and path == 0


@pytest.mark.parametrize("d", [100, 128])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 2049])
def test_exact_path(d, A):
    """one row to 64 in the last chunk of a segment; 2049 ids are two segments at 30 queries"""
    index, Q, ridx, _ = big(d)
    row = np.zeros((1, 3000), dtype=bool)
    row[0, np.random.default_rng(A).choice(3000, A, replace=False)] = True
    mo = np.zeros(30, dtype=np.int64)
    check(index, ridx, Q, 10, 64, row, lambda: index.search_batch_filtered_multi(Q, 10, 64, row, mo), exact=True)


def test_exact_path_grouped():
    index, Q, ridx, _ = big(128)
    rows, mo = two_rows(3000, 5), np.arange(30) % 2
    index.set_option("filter_exact_grouped", 1)
    check(index, ridx, Q, 10, 64, rows[mo], lambda: index.search_batch_filtered_multi(Q, 10, 64, rows, mo), exact=True)
    index.set_option("filter_exact_grouped", 0)


def test_deletions():
    import torch
    index, X, Q, ridx = build(600, 128, 8, 12)
    gone = np.flatnonzero(np.random.default_rng(6).random(600) < 0.1)
    index.mark_deleted(gone)
    alive = np.ones((1, 600), dtype=bool)
    alive[0, gone] = False
    path0 = lambda out: tuple(out) + (np.zeros(12, dtype=np.uint8),)
    check(index, ridx, Q, 10, 64, alive, lambda: path0(index.search_batch(Q, 10, 64)), what="search_batch")
    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(Q).to(dev)
    out = [torch.zeros(s, dtype=t, device=dev) for s, t in
           (((12, 10), torch.int32), ((12, 10), torch.float32), ((12,), torch.int32), ((12, 4), torch.int32))]
    ptrs = (dQ.data_ptr(), 12, 10, 64) + tuple(o.data_ptr() for o in out) + (0,)

    def device():
        index.search_batch_device(*ptrs)
        index.search_batch_device_finish(*ptrs)
        got = [o.cpu().numpy() for o in out]
        return path0((got[0].view(np.uint32), got[1], got[2].view(np.uint32), got[3]))
    check(index, ridx, Q, 10, 64, alive, device, what="device pointers")
    want = FR.graph(ridx, Q[0], 10, 64, lambda i: bool(alive[0][i]))["ids"]
    assert index.ann_by_vector(Q[0], 10, 64) == [int(x) for x in want]
    index.unmark_deleted(gone)
    with H.kernel_log() as log:
        index.search_batch(Q, 10, 64)
    assert set(log) == {"hx_search16_kernel<128, 1>"}, dict(log)


def test_live_snapshot():
    X, Q = rand_vectors(620, 100, 11) * 2 - 0.5, rand_vectors(8, 100, 12) * 2 - 0.5
    lab = np.random.default_rng(7).integers(0, 4, 620).astype(np.uint32)
    index = f16_index(X[:600], 8)
    index.set_labels(lab[:600])
    index.search_batch_filtered_range(Q, 10, 64, 1, 2)  # the snapshot is live from here on
    for i in range(600, 620):
        index.insert_vec(X[i], i % 2)
        index.set_labels(lab[i:i + 1], [i])
        a = ((lab[:i + 1] >= 1) & (lab[:i + 1] <= 2))[None]
        check(index, restated(index, X[:i + 1]), Q, 10, 64, a, lambda: index.search_batch_filtered_range(Q, 10, 64, 1, 2), what=str(i))


@pytest.mark.parametrize("d", [100, 128])
@pytest.mark.parametrize("what", ["subnormals", "largest"])
def test_range_of_f16(d, what):
    X, Q = rand_vectors(600, d, 7), rand_vectors(12, d, 8)
    if what == "subnormals":
        X, Q = X * np.float32(2.0**-18), Q * np.float32(2.0**-18)
        assert 0 < np.abs(widen(X)).max() < 2.0**-14
    else:
        s = np.float32(65504.0 / float(X.max()))
        X, Q = np.minimum(X * s, np.float32(65504)), Q * s
        X[np.unravel_index(X.argmax(), X.shape)] = 65504
    index = f16_index(X, 8)
    ridx = restated(index, X)
    rows, mo = two_rows(600)[:1], np.zeros(12, dtype=np.int64)
    ms = index.mask_set(rows)
    check(index, ridx, Q, 10, 64, rows, lambda: index.search_batch_filtered_set(Q, 10, 64, ms, mo), what=what)


def test_refusals_that_remain():
    index, X, Q, _ = build(600, 24, 8, 4)
    for call, args in [(index.search_batch_filtered, (Q, 5, 32, np.arange(100))), (index.search_batch_filtered_wide, (Q, 100, 200))]:
        with pytest.raises(H.HnswError) as e:
            call(*args)
        assert e.value.code == _lib.ERR_ARG and "rows_f16" in str(e.value)
