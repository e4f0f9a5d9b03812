"""One merge per committed pass of the lean f32 kernels (search_lean.hip, DESIGN.md 4a: a pass that commits its runner-up
claims p's slots first and merges the keys of both rows once) against the CPU oracle, through the C ABI: ids, distance
bits, counts and the three counters, and the kernel that is expected ran.  The fixtures are tests/one_merge_commit.py's
hand-made graphs; every graph first proves on the CPU replay that its rows provoke the states their names promise (the
assertions of tests/test_one_merge_commit_host.py).  f32 rows at d = 100 over a list of one register (ef 1 .. 4, 64) and
head + tail (65, 68, 128).  The tests hold any way of merging: they ask for the oracle's results, not for the mechanism."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from tests import one_merge_commit as OM
from tests.util import assert_search_equal, product_from_oracle

pytestmark = pytest.mark.gpu

CASES = OM.SCRIPTS + [("overflow", 64), ("overflow", 68)]


def kernel_of(ef):
    return "hx_lean_f32_kernel<100, %s, 4>" % ("Lst<1>" if ef <= 64 else "LstHT")


@pytest.mark.parametrize("kind,ef", CASES, ids=["%s-%d" % c for c in CASES])
def test_f32_100d(kind, ef):
    OM.assert_states(kind, ef)
    orc, rows, lv, qs, _ = OM.handmade(kind, ef)
    index = product_from_oracle(orc, rows, lv)
    what = "one merge %s ef=%d" % (kind, ef)
    with H.kernel_log() as log:
        got = index.search_batch(qs, OM.TOPN, ef)
    assert kernel_of(ef) in log, (what, kernel_of(ef), dict(log))
    assert_search_equal(got, orc.search_batch(qs, OM.TOPN, ef, nthreads=8), what)


@pytest.mark.parametrize("ef", OM.EFS)
def test_every_graph_at_every_ef(ef):
    """the graphs laid for one ef, searched with another: other states than the ones they were laid for, same oracle"""
    for kind, ef_laid in CASES:
        if ef_laid == ef:
            continue
        orc, rows, lv, qs, _ = OM.handmade(kind, ef_laid)
        index = product_from_oracle(orc, rows, lv)
        what = "one merge %s laid for ef=%d at ef=%d" % (kind, ef_laid, ef)
        assert_search_equal(index.search_batch(qs, OM.TOPN, ef), orc.search_batch(qs, OM.TOPN, ef, nthreads=8), what)


def first_launch(index, qs, ef):
    """hnsw_search_batch_device without its finish: what the kernel itself leaves -> (ids, counts, stats [nq, 4])"""
    import torch
    index.upload()
    nq, dev = qs.shape[0], torch.device("cuda:0")
    dQ = torch.from_numpy(qs).to(dev)
    d_ids = torch.empty((nq, OM.TOPN), dtype=torch.int32, device=dev)
    d_dists = torch.empty((nq, OM.TOPN), dtype=torch.float32, device=dev)
    d_counts = torch.empty(nq, dtype=torch.int32, device=dev)
    d_stats = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    try:
        index.search_batch_device(dQ.data_ptr(), nq, OM.TOPN, ef, d_ids.data_ptr(), d_dists.data_ptr(), d_counts.data_ptr(),
                                  d_stats.data_ptr(), 0)
    except H.HnswError:
        pass  # (a flagged query; the arrays are the kernel's)
    torch.cuda.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_counts.cpu().numpy(), d_stats.cpu().numpy()


@pytest.mark.parametrize("ef", (64, 65, 68, 128))
def test_one_merge_of_64_survivors(ef):
    """c's and p's rows of 32 fresh ids into a list of three entries: the big merge with every lane a survivor"""
    _, orc, rows, lv = OM.full_rows()
    index = product_from_oracle(orc, rows, lv)
    qs = np.zeros((2, OM.D), dtype=np.float32)
    qs[1, 0] = 250.0
    with H.kernel_log() as log:
        got = index.search_batch(qs, OM.TOPN, ef)
    assert kernel_of(ef) in log, dict(log)
    assert_search_equal(got, orc.search_batch(qs, OM.TOPN, ef), "64 survivors ef=%d" % ef)


@pytest.mark.parametrize("ef", (64, 68))
@pytest.mark.parametrize("which", list(OM.VISITED))
def test_the_visited_limit_reached_by_the_claims_of_p(which, ef):
    """the first launch's own words: no overflow just under the limit; reached by p's claims, the status and the
    counters of both expansions; reached by c's claims, those of c's alone.  The host entry then runs the query again
    with a larger table and answers as the oracle does."""
    _, orc, rows, lv, want = OM.visited(which)
    index = product_from_oracle(orc, rows, lv)
    q0 = np.zeros((1, OM.D), dtype=np.float32)
    o = orc.search_batch(q0, OM.TOPN, ef)
    ids, counts, stats = first_launch(index, q0, ef)
    if want is None:
        assert stats[0, 3] == 0 and stats[0, :3].tolist() == o[3][0].tolist() and np.array_equal(ids, o[0])
    else:
        assert stats[0].tolist() == list(want) + [H._lib.ERR_OVERFLOW], (which, ef, stats[0], want)
        assert counts[0] == 0 and (ids[0] == H._lib.UINT32_MAX).all()
    assert_search_equal(index.search_batch(q0, OM.TOPN, ef), o, "visited limit %s ef=%d" % (which, ef))


@pytest.mark.parametrize("ef", (64, 68))
@pytest.mark.parametrize("side", ("clean", "c", "p", "both"))
def test_a_nan_distance_of_a_neighbour(side, ef):
    """a NaN distance of a fresh neighbour of c, of the committed p, of both: the NaN status, no result and the counters
    up to and with the expansion that met it (c's is met before p is committed); without one, the oracle's answer"""
    _, orc, rows, lv, q, counters = OM.nan_case(side)
    index = product_from_oracle(orc, rows, lv)
    ids, counts, stats = first_launch(index, q, ef)
    if side == "clean":
        assert stats[0, 3] == 0
        assert_search_equal(index.search_batch(q, OM.TOPN, ef), orc.search_batch(q, OM.TOPN, ef), "all distances inf ef=%d" % ef)
        return
    want = [counters[0] + 1, counters[1], counters[2], H._lib.ERR_NAN_INPUT]
    assert stats[0].tolist() == want, (side, ef, stats[0], want)
    assert counts[0] == 0 and (ids[0] == H._lib.UINT32_MAX).all()
    with pytest.raises(H.HnswError) as e:
        index.search_batch(q, OM.TOPN, ef)
    assert e.value.code == H._lib.ERR_NAN_INPUT
