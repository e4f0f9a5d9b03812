"""The frontier of the lean f32 kernels' list (search_lean.hip, DESIGN.md 4a: c, p and the pair requested ahead come
from the first four unexpanded keys, found once per pass) against the CPU oracle, through the C ABI: ids, distance bits,
counts and the three counters, and the kernel that is expected ran.  The fixtures are tests/frontier.py's hand-made
graphs; every graph first proves on the CPU replay that its rows provoke the states their names promise (the assertions
of tests/test_frontier_host.py).  f32 rows at d = 100 over a list of one register (ef 1 .. 4, 64) and head + tail (65, 68,
128).  The tests hold any way of picking: they ask for the oracle's results, not for the mechanism."""
import pytest

import hnsw_rs_amd as H
from tests import frontier as FR
from tests.util import assert_search_equal, product_from_oracle

pytestmark = pytest.mark.gpu

CASES = FR.SCRIPTS + [("overflow", 64), ("overflow", 68)]


def kernel_of(ef):
    return "hx_lean_f32_kernel<100, %s, 4>" % ("Lst<1>" if ef <= 64 else "LstHT")


@pytest.mark.parametrize("kind,ef", CASES, ids=["%s-%d" % c for c in CASES])
def test_f32_100d(kind, ef):
    FR.assert_states(kind, ef)
    orc, rows, lv, qs, _ = FR.handmade(kind, ef)
    index = product_from_oracle(orc, rows, lv)
    what = "frontier %s ef=%d" % (kind, ef)
    with H.kernel_log() as log:
        got = index.search_batch(qs, FR.TOPN, ef)
    assert kernel_of(ef) in log, (what, kernel_of(ef), dict(log))
    assert_search_equal(got, orc.search_batch(qs, FR.TOPN, ef, nthreads=8), what)


@pytest.mark.parametrize("ef", (1, 2, 3, 4, 64, 65, 68, 128))
def test_every_graph_at_every_ef(ef):
    """the graphs laid for one ef, searched with another: other states than the ones they were laid for, same oracle"""
    for kind, ef_laid in CASES:
        if ef_laid == ef:
            continue
        orc, rows, lv, qs, _ = FR.handmade(kind, ef_laid)
        index = product_from_oracle(orc, rows, lv)
        what = "frontier %s laid for ef=%d at ef=%d" % (kind, ef_laid, ef)
        assert_search_equal(index.search_batch(qs, FR.TOPN, ef), orc.search_batch(qs, FR.TOPN, ef, nthreads=8), what)
