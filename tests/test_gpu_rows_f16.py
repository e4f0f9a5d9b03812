"""The search over f16-resident rows (option "rows_f16", search_rows16.hip) against the plain f32
oracle over the widened rows X16 = X.astype(float16).astype(float32): ids, distance bits and traversal counters.  Every
test needs an MI355X and fails on a library without the option."""
import threading

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import assert_search_equal, oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu


def widen(X):
    return X.astype(np.float16).astype(np.float32)


def both(X, m, threads=4):
    """the index under the option over X, the oracle over X16 on the same graph, the levels"""
    lv = O.draw_levels(len(X), m, 3)
    index = H.HNSW.new(m, 32, X.shape[1], H.VEC_F32)
    index.set_option("rows_f16", 1)
    index.insert_bulk(X, threads, False, levels=lv)
    return index, oracle_from_product(index, widen(X), lv), lv


def rows_and_queries(n, d, nq=40):
    return rand_vectors(n, d, 100 + d) * 2 - 0.5, rand_vectors(nq, d, 200 + d) * 2 - 0.5


def kernel_for(d, ef):
    """the instantiation of hx_search16_kernel<DS, R> the launcher picks (named in tests/test_rows_f16_host.py)"""
    r = 1 if ef <= 64 else 2 if ef <= 128 else 4 if ef <= 256 else 8 if ef <= 512 else 16
    return "hx_search16_kernel<%d, %d>" % (d if d in (128, 256, 768) and r < 16 else 0, r)


def check(index, orc, Q, k, ef):
    with H.kernel_log() as log:
        got = index.search_batch(Q, k, ef)
    assert set(log) == {kernel_for(Q.shape[1], ef)}, dict(log)
    assert_search_equal(got, orc.search_batch(Q, k, ef), "d=%d ef=%d" % (Q.shape[1], ef))


@pytest.mark.parametrize("d", [1, 7, 8, 9, 64, 100, 128, 136, 192, 256, 768])
def test_every_dimension_path(d):
    """both sides of the 8-element piece and of the 64-element line, every cooperative width, one line-sized width that
    is not instantiated (192) and one just off a line (136)"""
    X, Q = rows_and_queries(600, d)
    index, orc, _ = both(X, 8)
    for ef in (1, 17, 64):
        check(index, orc, Q, 10, ef)


@pytest.mark.parametrize("d", [24, 128, 256, 768])
def test_every_list_width_of_every_gather(d):
    X, Q = rows_and_queries(600, d)
    index, orc, _ = both(X, 8)
    for ef in (100, 200, 300):  # two, four and eight list registers
        check(index, orc, Q, 10, ef)


@pytest.mark.parametrize("d", [128, 256])
def test_more_than_32_wanted_rows_in_a_pass(d):
    X, Q = rows_and_queries(3000, d)
    index, orc, _ = both(X, 16)  # S0 = 32: the candidate's and the runner-up's rows together
    assert_search_equal(index.search_batch(Q, 10, 64), orc.search_batch(Q, 10, 64))


@pytest.fixture(scope="module", params=[24, 128])
def wide(request):
    X, Q = rows_and_queries(3000, request.param)
    return both(X, 8) + (Q,)


@pytest.mark.parametrize("ef", [65, 300, 513, 1024])
def test_list_widths(wide, ef):
    index, orc, _, Q = wide
    check(index, orc, Q, 100, ef)


def test_ef_above_1024_is_refused(wide):
    index, _, _, Q = wide
    with pytest.raises(H.HnswError) as e:
        index.search_batch(Q, 100, 1025)
    assert e.value.code == _lib.ERR_ARG and "rows_f16" in str(e.value)


@pytest.mark.parametrize("d", [128, 100])
@pytest.mark.parametrize("what", ["subnormals", "largest"])
def test_range_of_f16(d, what):
    """rows of f16 subnormals (a widening that flushes them fails) and rows whose largest element is 65504"""
    X, Q = rand_vectors(600, d, 7), rand_vectors(40, d, 8)
    if what == "subnormals":
        X, Q = X * np.float32(2.0**-18), Q * np.float32(2.0**-18)
        assert 0 < np.abs(widen(X)).max() < 2.0**-14
    else:
        s = np.float32(65504.0 / float(X.max()))
        X, Q = np.minimum(X * s, np.float32(65504)), Q * s
        X[np.unravel_index(X.argmax(), X.shape)] = 65504
    index, orc, _ = both(X, 8)
    assert_search_equal(index.search_batch(Q, 10, 64), orc.search_batch(Q, 10, 64), what)


@pytest.mark.parametrize("d", [100, 768])
def test_snapshot_stores_two_bytes_per_element(d):
    X, _ = rows_and_queries(600, d)
    index, _, lv = both(X, 8, threads=1)
    plain = H.HNSW.new(8, 32, d, H.VEC_F32).insert_bulk(widen(X), 1, False, levels=lv)
    index.upload(), plain.upload()
    saved = len(X) * (((4 * d + 15) & ~15) - 16 * -(-2 * d // 16))
    assert saved > 0 and index.stat("snapshot_bytes") == plain.stat("snapshot_bytes") - saved


def test_live_index():
    import torch
    d, k, ef = 100, 10, 64
    X, Q = rows_and_queries(620, d)
    index, orc, lv = both(X[:600], 8)
    want = orc.search_batch(Q, k, ef)
    assert_search_equal(index.search_batch(Q, k, ef), want)
    # the device-pointer entry and its completion
    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(Q).to(dev)
    out = [torch.zeros(s, dtype=t, device=dev) for s, t in
           (((40, k), torch.int32), ((40, k), torch.float32), ((40,), torch.int32), ((40, 4), torch.int32))]
    ptrs = (dQ.data_ptr(), 40, k, ef) + tuple(o.data_ptr() for o in out) + (0,)
    index.search_batch_device(*ptrs)
    index.search_batch_device_finish(*ptrs)
    got = [o.cpu().numpy() for o in out]
    assert_search_equal((got[0].view(np.uint32), got[1], got[2].view(np.uint32), got[3]), want, "device pointers")
    # the one-query entry from 8 threads
    answers = [None] * 40
    def worker(t):
        for i in range(t, 40, 8):
            answers[i] = index.ann_by_vector(Q[i], k, ef)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    [t.start() for t in threads], [t.join() for t in threads]
    assert answers == [[int(x) for x in row] for row in want[0]]
    # insert_vec on the live snapshot, a search after each
    for i in range(600, 620):
        index.insert_vec(X[i], i % 2)
        lv = np.append(lv, np.uint8(i % 2))
        orc = oracle_from_product(index, widen(X[:i + 1]), lv)
        assert_search_equal(index.search_batch(Q, k, ef), orc.search_batch(Q, k, ef), "after insert %d" % i)


def test_recall_is_that_of_the_f32_index():
    """f16 rounding moves a distance by about 2^-11 relative, far below these rows' neighbour gaps:
    recall@10 against float64 ground truth over the UNROUNDED rows stays within 0.01 of the plain f32 index's.  (Checked on
    the CPU first, single-threaded builds, the f32 oracle on each graph: 0.932 over X16 against 0.933 over X.)"""
    g = np.random.Generator(np.random.PCG64(5))
    X, Q = g.standard_normal((5000, 128), dtype=np.float32), g.standard_normal((100, 128), dtype=np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    d2 = (Q64**2).sum(1)[:, None] - 2 * Q64 @ X64.T + (X64**2).sum(1)[None, :]
    truth = np.argsort(d2, axis=1, kind="stable")[:, :10]
    lv = O.draw_levels(len(X), 16, 3)
    plain = H.HNSW.new(16, 32, 128, H.VEC_F32).insert_bulk(X, 1, False, levels=lv)
    recall = lambda index: np.mean([len(set(a) & set(b)) for a, b in zip(index.search_batch(Q, 10, 100)[0], truth)]) / 10
    r16, r32 = recall(both(X, 16, threads=1)[0]), recall(plain)
    print("recall@10: f16 rows %.4f, f32 rows %.4f" % (r16, r32))
    assert abs(r16 - r32) <= 0.01
