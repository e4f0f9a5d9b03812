"""hnsw_brute_force_fast over f16-resident rows (option "rows_f16"; brute_mfma16.hip) against the
exact scan of a plain f32 index over the widened rows X16 = X.astype(float16).astype(float32) -- hnsw_brute_force, which
tests/test_gpu_ground_truth.py pins to the oracle: ids and distance bits are equal on every query where the scores are
exact (integer rows) and on every query whose margin (tests/ground_truth_inputs.py, float64) exceeds the declared 4 E.
Every case asserts with the launch log which kernels ran, and fails on a library that refuses the call."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from hnsw_rs_amd import eval as E
from oracle import oracle_py as O
from tests import ground_truth_inputs as G

pytestmark = pytest.mark.gpu


def widen(X):
    return X.astype(np.float16).astype(np.float32)


def flat(X, f16):
    """an index without a graph (a case costs its scans and nothing else), under the option or plain"""
    N, d = X.shape
    idx = H.HNSW.new(8, 16, d, H.VEC_F32)
    if f16:
        idx.set_option("rows_f16", 1)
    idx.import_points(X, np.zeros(N, dtype=np.uint8))
    idx.import_layer(0, np.arange(N, dtype=np.uint32), np.zeros(N + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    idx.set_ep(0)
    idx.upload()
    return idx


def kernels(d):
    """two 32-query column tiles per workgroup while their planes fit in LDS (d <= 416), else one"""
    return {"hx_row_norms16_kernel", "hx_brute_mfma16_kernel<%d>" % (2 if d <= 416 else 1), "hx_pair_distance16_kernel"}


def same(got, want, what):
    bad = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d queries differ, first %d: got %s %s want %s %s" % (
        what, bad.size, len(got[0]), bad[0], got[0][bad[0]], got[1][bad[0]], want[0][bad[0]], want[1][bad[0]])


def fast(X, Q, k=G.K):
    idx = flat(X, True)
    with H.kernel_log() as log:
        got = idx.brute_force_fast(Q, k)
    return got, set(log)


@pytest.mark.parametrize("family", ["ints", "late"])
@pytest.mark.parametrize("d", [4, 8, 12, 24, 100, 128, 768])
def test_exact_on_every_query_of_integer_rows(d, family):
    """below one 16-byte piece, one piece, a half piece of padding, an odd piece count, 100, a full line, the widest; 9000
    rows are two segments and no multiple of 32, 70 queries three column tiles with the last one partial; `late` makes
    a lane give up the tied row of the highest id.  Integers are binary16 values and every sum is exact."""
    X, Q = G.ints(9000, d, hi=3, nq=70) if family == "ints" else G.late(9000, d)
    got, log = fast(X, Q)
    assert log == kernels(d), log
    same(got, flat(X, False).brute_force(Q, G.K), "%s d=%d" % (family, d))


EXACT_PATH = {"hx_row_norms16_kernel", "hx_filt_compact_kernel", "hx_filt_merge_kernel"}


@pytest.mark.parametrize("rows", ["as drawn", "no subnormals"])
@pytest.mark.parametrize("N,d", [(5000, 128), (9000, 68), (3000, 768), (2000, 100)])
def test_exact_on_every_safe_query(N, d, rows):
    """a query is safe when its margin over the widened rows exceeds 4 (the screen's declared bound is 4 E); all are.
    Standard normal rows AS DRAWN hold a few elements below 2^-14, binary16 subnormals, so the call takes the exact path
    (asserted); with those elements set to zero the screen itself answers, and is held to its bound."""
    X, Q = G.gauss(N, d, 0)
    X16 = widen(X)
    tiny = (X16 != 0) & (np.abs(X16) < 2.0 ** -14)
    assert tiny.any()
    if rows == "no subnormals":
        X16[tiny] = 0
    want = flat(X16, False).brute_force(Q, G.K)
    margin = G.margin(X16, Q, G.K, want[0])
    print("gauss(%d, %d, 0), %s: smallest margin %.3g" % (N, d, rows, margin.min()))
    assert (margin > 4).mean() == 1.0
    got, log = fast(X if rows == "as drawn" else X16, Q)
    assert log == (kernels(d) if rows == "no subnormals" else EXACT_PATH | {"hx_filt16_scan_kernel<%d>" % (d if d in (128, 768) else 0)}), log
    same(got, want, "gauss(%d, %d, 0), %s" % (N, d, rows))


@pytest.mark.parametrize("case", ["subnormal row", "query of 2^50"])
def test_a_call_outside_the_range_takes_the_exact_scan(case):
    """rows the screen serves (the test above), then ONE element a binary16 subnormal, or one query component 2^50"""
    X, Q = G.gauss(2000, 100, 0)
    X = widen(X)
    X[np.abs(X) < 2.0 ** -14] = 0
    if case == "subnormal row":
        X[1234, 5] = 2.0 ** -20
    else:
        Q[3, 2] = 2.0 ** 50
    got, log = fast(X, Q)
    assert log == EXACT_PATH | {"hx_filt16_scan_kernel<0>"}, log
    same(got, flat(X, False).brute_force(Q, G.K), case)


def test_statuses():
    X, Q = G.ints(300, 8, 3)
    idx = flat(X, True)
    for k, q, code in [(13, Q, _lib.ERR_ARG), (G.K, np.where(np.arange(8) == 5, np.nan, Q), _lib.ERR_NAN_INPUT)]:
        with pytest.raises(H.HnswError) as e:
            idx.brute_force_fast(q, k)
        assert e.value.code == code, e.value
    idx.mark_deleted([7])
    with pytest.raises(H.HnswError) as e:
        idx.brute_force_fast(Q, G.K)
    assert e.value.code == _lib.ERR_ARG and "deleted" in str(e.value)


def test_the_harness_measures_recall_on_such_an_index():
    X, Q = G.gauss(2000, 24, 0)
    idx = H.HNSW.new(8, 32, 24, H.VEC_F32)
    idx.set_option("rows_f16", 1)
    idx.insert_bulk(X, 4, False, levels=O.draw_levels(2000, 8, 3))
    with H.kernel_log() as log:
        recall = E.recall_at(idx, Q, 10, 32)
    assert "hx_row_norms16_kernel" in log, dict(log)  # (either path of the truth is right)
    truth, ids = idx.brute_force_fast(Q, 10)[0], idx.search_batch(Q, 10, 32)[0]
    assert recall == sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / 640.0
