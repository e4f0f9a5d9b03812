"""The two exhaustive scans behind every recall figure, held to the oracle at their edges.

hnsw_brute_force (hx_brute_kernel<kind>, nseg = min(512, ceil(N / 2048)) segments merged on the host) must equal
orc.brute_force in ids and distance bits everywhere.  hnsw_brute_force_fast (hx_row_norms_kernel, hx_brute_mfma_kernel,
hx_pair_distance_kernel) must equal it wherever the screen's order is decided: on the ints and dups families of
tests/ground_truth_inputs.py (exact scores, massive ties) on every query, on the gauss families on every query that
safe() proves (at least 0.9 of them, asserted here and in tests/test_ground_truth_inputs.py).  Beyond the bound a query
keeps the contract of test_what_holds_beyond_the_bound and no recall figure.

Every index is built without a graph (import_points with levels 0, an empty layer 0, set_ep(0)) on both sides: a case
costs a scan and nothing else.
"""
import time

import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import ground_truth_inputs as G
from tests.kernel_matrix import edge_queries
from tests.test_ground_truth_inputs import family, flat_oracle

pytestmark = pytest.mark.gpu

Q8, F32 = H.VEC_QUANT8, H.VEC_F32
FAST_KERNELS = {"hx_row_norms_kernel", "hx_brute_mfma_kernel", "hx_pair_distance_kernel"}


def flat_product(X, kind=F32, cosine=False):
    N, d = X.shape
    idx = H.HNSW.new(8, 16, d, kind)
    if cosine:
        idx.set_option("metric_cosine", 1)
    idx.import_points(X, np.zeros(N, dtype=np.uint8))
    idx.import_layer(0, np.arange(N, dtype=np.uint32), np.zeros(N + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    idx.set_ep(0)
    idx.upload()
    return idx


def assert_same(got, want, what):
    g_ids, g_d = got
    w_ids, w_d = want
    bad = np.nonzero((g_ids != w_ids).any(axis=1) | (g_d.view(np.uint32) != w_d.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d queries differ, first %d: got %s %s want %s %s" % (
        what, bad.size, g_ids.shape[0], bad[0], g_ids[bad[0]], g_d[bad[0]], w_ids[bad[0]], w_d[bad[0]])


def exact_check(idx, orc, Q, k, what):
    with H.kernel_log() as log:
        got = idx.brute_force(Q, k)
    assert set(log) == {"hx_brute_kernel<%d>" % idx.vec_kind}, (what, dict(log))
    assert_same(got, orc.brute_force(Q, k, nthreads=8), "%s k=%d" % (what, k))


def fast_check(X, Q, k=G.K, what=""):
    """brute_force_fast == the oracle on every query, through exactly the three kernels"""
    idx, orc = flat_product(X), flat_oracle(X)
    with H.kernel_log() as log:
        got = idx.brute_force_fast(Q, k)
    assert set(log) == FAST_KERNELS, (what, dict(log))
    assert_same(got, orc.brute_force(Q, k, nthreads=8), "%s N=%d d=%d nq=%d k=%d" % ((what,) + X.shape + (len(Q), k)))


# ---- the exact scan ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [Q8, F32], ids=["q8", "f32"])
@pytest.mark.parametrize("d", [8, 40])
@pytest.mark.parametrize("N", [2048, 2049, 4097])
def test_exact_scan_segment_boundaries(N, d, kind):
    """one, two and three segments: the host merge of the per-segment lists, at k = 1, 10 and the largest"""
    X, Q = G.gauss(N, d, 0, nq=16)
    Q = np.concatenate([Q, edge_queries(X, kind)])
    idx, orc = flat_product(X, kind), flat_oracle(X, kind)
    for k in (1, 10, 64):
        exact_check(idx, orc, Q, k, "segments N=%d d=%d kind=%d" % (N, d, kind))


@pytest.mark.parametrize("kind", [Q8, F32], ids=["q8", "f32"])
def test_exact_scan_ties_across_segments(kind):
    """rows of zeros and ones: tie groups far larger than k that span the segment boundaries; ids alone decide"""
    X, Q = G.ints(4097, 8, 1)
    exact_check(flat_product(X, kind), flat_oracle(X, kind), Q, 64, "ties kind=%d" % kind)


@pytest.mark.parametrize("kind", [Q8, F32], ids=["q8", "f32"])
def test_exact_scan_second_query_batch(kind):
    """2049 queries: the last one is a launch of its own and must land in row 2048"""
    X, Q = G.gauss(300, 8, 0, nq=2049)
    exact_check(flat_product(X, kind), flat_oracle(X, kind), Q, 10, "second batch kind=%d" % kind)


@pytest.mark.parametrize("kind", [Q8, F32], ids=["q8", "f32"])
def test_exact_scan_pads_beyond_the_points(kind):
    X, Q = G.gauss(5, 8, 0, nq=4)
    idx, orc = flat_product(X, kind), flat_oracle(X, kind)
    exact_check(idx, orc, Q, 64, "padding kind=%d" % kind)
    ids, dist = idx.brute_force(Q, 64)
    assert (ids[:, 5:] == O.UINT32_MAX).all() and np.isposinf(dist[:, 5:]).all() and (ids[:, :5] < 5).all()


def test_exact_scan_at_the_segment_cap():
    """N = 2048 * 512 + 1: ceil(N / 2048) = 513 segments are capped at 512 of 2049 rows.  A row repeated in the middle
    and at the very end ties with the query's own row across the first, a middle and the last segment."""
    N = 2048 * 512 + 1
    X, Q = G.gauss(N, 4, 0, nq=4)
    X[N // 2] = X[N - 1] = X[0]
    Q[0] = X[0]
    t = time.time()
    idx, orc = flat_product(X, F32), flat_oracle(X, F32)
    print("segment cap: import and upload of %d rows %.2f s" % (N, time.time() - t))
    exact_check(idx, orc, Q, 10, "segment cap")
    assert idx.brute_force(Q[:1], 3)[0].tolist() == [[0, N // 2, N - 1]]


# ---- the MFMA scan -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [4, 8, 64, 68, 72, 132, 376, 380])
def test_mfma_scan_row_widths(d):
    """one piece with the upper half of the wave idle (4), one stage exactly (64), the second stage with an odd and an
    even number of pieces (68, 72), three stages (132), the last width under and the first over the 48-KiB opt-in"""
    fast_check(*G.ints(300, d, 3), what="row width")


def test_mfma_scan_at_the_lds_limit():
    """d = 1272 stages 32 x 1276 floats + 128 norms = 160 KiB exactly, the largest the host accepts; d = 1276 is
    refused"""
    fast_check(*G.ints(64, 1272, 3), what="160 KiB")
    X, Q = G.ints(64, 1276, 3)
    with pytest.raises(H.HnswError):
        flat_product(X).brute_force_fast(Q, G.K)


@pytest.mark.parametrize("N", [1, 11, 19, 20, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 12289])
def test_mfma_scan_point_tile_and_segment_remainders(N):
    """fewer points than k (1, 11) and than k + 8 (19) with the oracle's padding, a last tile of 1 .. 32 rows, waves
    with nothing to do (33), and at 8193 / 12289 segments of 4097 rows that start at rows 4097 and 8194"""
    fast_check(*G.ints(N, 8, 3), what="remainders")


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 2048, 2049])
def test_mfma_scan_query_tiles_and_batches(nq):
    fast_check(*G.ints(300, 8, 3, nq=nq), what="query tiles")


def test_mfma_scan_segment_cap_and_second_batch():
    """2049 queries are 64 tiles: 768 / 64 = 12 segments cap N / 4096 = 13; the second batch (one query, one tile) runs
    with the same 12.  Rows of 8^4 values: every query has about 13 exact copies among the rows, spread over the
    segments, and its k lowest ids are the answer."""
    fast_check(*G.ints(53253, 4, 7, nq=2049), what="segment cap")


@pytest.mark.parametrize("k", [1, 12])
def test_mfma_scan_smallest_and_largest_k(k):
    fast_check(*G.ints(300, 8, 3), k=k, what="k")


@pytest.mark.parametrize("k", [0, 13])
def test_mfma_scan_refuses_other_k(k):
    X, Q = G.ints(300, 8, 3)
    with pytest.raises(H.HnswError):
        flat_product(X).brute_force_fast(Q, k)


def test_mfma_scan_ties_of_repeated_rows():
    """40 copies of the nearest row at scattered ids: bit-equal scores, the lowest ids win"""
    fast_check(*G.dups(5000, 64), what="dups")


def test_mfma_scan_ties_of_integer_rows():
    fast_check(*G.ints(5000, 8, 3), what="ints ties")


@pytest.mark.parametrize("N", [300, 5000])
def test_mfma_scan_keeps_the_lowest_ids_when_a_better_row_comes_late(N):
    """a lane's candidate list is full of tied rows when a nearer row arrives: the tied row of the highest id has to
    go, since the answer continues with the lowest ids"""
    fast_check(*G.late(N, 8), what="late")


def beyond_the_bound(idx, orc, X, Q, got, exact_d, what):
    """the whole contract of a query the bound does not cover: k distinct stored ids, no padding, the reference's own
    distances of those ids, in (dist, id) order, none better than the exact answer at the same position"""
    ids, dist = got
    N = X.shape[0]
    for qi in range(Q.shape[0]):
        i, dd = ids[qi], dist[qi]
        assert (i < N).all() and len(set(i.tolist())) == len(i), (what, qi, i)
        assert np.array_equal(dd.view(np.uint32), orc.distance_batch(Q[qi], i).view(np.uint32)), (what, qi)
        keys = list(zip(dd.tolist(), i.tolist()))
        assert keys == sorted(keys), (what, qi, keys)
        assert (dd >= exact_d[qi]).all(), (what, qi, dd, exact_d[qi])


@pytest.mark.parametrize("N,d,offset", G.PRECISION)
def test_mfma_scan_is_exact_on_every_safe_query(N, d, offset):
    """the guarantee: wherever the float64 predicate proves that f32 rounding cannot push one of the oracle's k out of
    the screen's k + 8, ids and distance bits are the oracle's; the tight offsets leave a bf16 or tf32 screen no room
    (tests/test_ground_truth_inputs.py)"""
    X, Q, w_ids, w_d = family(N, d, offset)
    safe = G.safe(X, Q, G.K, w_ids)
    print("gauss(%d, %d, %g): safe share %.3f" % (N, d, offset, safe.mean()))
    assert safe.mean() >= G.SAFE_SHARE
    idx = flat_product(X)
    with H.kernel_log() as log:
        g_ids, g_d = idx.brute_force_fast(Q, G.K)
    assert set(log) == FAST_KERNELS, dict(log)
    assert_same((g_ids[safe], g_d[safe]), (w_ids[safe], w_d[safe]), "safe queries of gauss(%d, %d, %g)" % (N, d, offset))
    print("  the other %d queries: %d equal the oracle" % ((~safe).sum(), (g_ids[~safe] == w_ids[~safe]).all(axis=1).sum()))
    beyond_the_bound(idx, flat_oracle(X), X, Q[~safe], (g_ids[~safe], g_d[~safe]), w_d[~safe], "unsafe queries")


def test_what_holds_beyond_the_bound():
    """offset 100: no query is safe (asserted in tests/test_ground_truth_inputs.py); no recall is asserted"""
    X, Q, w_ids, w_d = family(*G.BEYOND)
    assert not G.safe(X, Q, G.K, w_ids).any()
    idx = flat_product(X)
    beyond_the_bound(idx, flat_oracle(X), X, Q, idx.brute_force_fast(Q, G.K), w_d, "gauss%r" % (G.BEYOND,))


def test_mfma_scan_under_the_cosine_option():
    """unit rows, metric_cosine = 1: the fast scan equals the product's own exact scan under the same option (which
    tests/test_gpu_configs.py holds to the oracle)"""
    X, Q = G.gauss(3000, 64, 0)
    X /= np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))[:, None].astype(np.float32)
    idx = flat_product(X, cosine=True)
    with H.kernel_log() as log:
        got = idx.brute_force_fast(Q, G.K)
    assert FAST_KERNELS <= set(log) and "hx_normalise_rows_kernel" in log, dict(log)
    assert_same(got, idx.brute_force(Q, G.K), "cosine")


def test_mfma_scan_reports_a_nan_query():
    X, Q = G.ints(300, 8, 3)
    Q[33, 5] = np.nan
    with pytest.raises(H.HnswError):
        flat_product(X).brute_force_fast(Q, G.K)
