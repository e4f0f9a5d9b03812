"""The front of a query in the lean f32 kernels against the CPU oracle, through hnsw_search_batch_device: ids, distance
bits, counts, n_dist, n_exp, sum_deg and the status, at ef 10 and 64 (one list register) and 68 (head + tail).  The
fixtures are tests/front_of_query.py's; every case first proves on the oracle that it has the pattern its name promises
(the assertions of tests/test_front_of_query_host.py).  Where the reference panics -- the distance of a stored row the
walk evaluates is a NaN: + infinity in the row and in the query, a NaN itself no index holds -- the expectation is stated
there (EXPECT_NAN): the status for every query, count 0, ids all ones, and the counters the reference had reached."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import front_of_query as FQ
from tests import numeric_range as NR
from tests.util import assert_search_equal

pytestmark = pytest.mark.gpu

LIST_OF = {10: "Lst<1>", 64: "Lst<1>", 68: "LstHT"}


def search_device(idx, qs, ef, finish=True, shift=0):
    """hnsw_search_batch_device (+ _finish) on torch buffers -> (ids, dists, counts, stats) as numpy, the log.
    shift: floats between a 16-byte boundary and the first query"""
    import torch
    dev = torch.device("cuda:0")
    nq = len(qs)
    idx.search_batch(qs[:1], FQ.TOPN, ef)  # (the first call uploads the snapshot)
    flat = torch.zeros(qs.size + shift, dtype=torch.float32, device=dev)
    dQ = flat[shift:]
    dQ.copy_(torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32).reshape(-1)))
    assert dQ.data_ptr() % 16 == 4 * shift
    ids = torch.full((nq, FQ.TOPN), 7, dtype=torch.int32, device=dev)
    dd = torch.full((nq, FQ.TOPN), -1.0, dtype=torch.float32, device=dev)
    cnt = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    st = torch.full((nq, 4), 7, dtype=torch.int32, device=dev)
    args = (dQ.data_ptr(), nq, FQ.TOPN, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0)
    with H.kernel_log() as log:
        idx.search_batch_device(*args)
        if finish:
            idx.search_batch_device_finish(*args)
    torch.cuda.synchronize()
    return (ids.cpu().numpy().view(np.uint32), dd.cpu().numpy(), cnt.cpu().numpy().view(np.uint32),
            st.cpu().numpy().astype(np.int64)), dict(log)


@pytest.mark.parametrize("ef", FQ.EFS)
@pytest.mark.parametrize("name", sorted(FQ.CASES))
def test_front_of_query(name, ef):
    FQ.assert_pattern(name)
    c, _ = FQ.fixture(name)
    what = "%s ef=%d" % (name, ef)
    got, log = search_device(FQ.product(name), c.queries, ef)
    assert "hx_lean_f32_kernel<100, %s, 4>" % LIST_OF[ef] in log, (what, log)
    assert_search_equal(got, FQ.expected(name, ef), what)
    assert (got[3][:, 3] == 0).all(), (what, got[3][:, 3])


@pytest.mark.parametrize("ef", FQ.EFS)
@pytest.mark.parametrize("name", sorted(FQ.NAN_CASES))
def test_nan_distance_of_a_stored_row(name, ef):
    FQ.assert_panics(name)
    c, _ = FQ.fixture(name)
    what = "%s ef=%d" % (name, ef)
    idx = FQ.product(name)
    E = H._lib.ERR_NAN_INPUT
    with NR.unchecked() as rcs:
        (ids, _, counts, stats), log = search_device(idx, c.queries, ef)
    assert [rc for rc in rcs if rc] == [E, E], (what, rcs)  # the warm-up call and the finish
    assert "hx_lean_f32_kernel<100, %s, 4>" % LIST_OF[ef] in log, (what, log)
    assert (stats[:, 3] == E).all(), (what, stats[:, 3])
    assert (counts == 0).all() and (ids == O.UINT32_MAX).all(), (what, counts, ids[:2])
    assert (stats[:, :3] == np.array(FQ.EXPECT_NAN[name])).all(), (what, stats[:2], FQ.EXPECT_NAN[name])


@pytest.mark.parametrize("ef", FQ.EFS)
@pytest.mark.parametrize("shift", (1, 2, 3))
def test_query_aligned_as_its_floats(shift, ef):
    """load_query_f32 takes the query in 16-byte pieces from an address that need only be 4-byte aligned: query
    buffers that start one, two and three floats behind a 16-byte boundary (rows of 100 floats keep that offset)"""
    name = "three_layers"
    c, _ = FQ.fixture(name)
    got, log = search_device(FQ.product(name), c.queries, ef, shift=shift)
    assert "hx_lean_f32_kernel<100, %s, 4>" % LIST_OF[ef] in log, (shift, ef, log)
    assert_search_equal(got, FQ.expected(name, ef), "shift=%d ef=%d" % (shift, ef))
