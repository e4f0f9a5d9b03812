"""The lean f32 kernel's handling of a runner-up's miss (search_lean.hip, DESIGN.md 4a: the follow-up pass's rows are
requested before c's merge, and a runner-up that is foreseen as the runner-up again keeps its distances) against the
CPU oracle, through the C ABI: ids, distance bits, counts and the three counters.  f32 rows at d = 100.  The fixtures
are tests/runner_up_miss.py's; every hand-made graph first proves on the CPU replay that it has the miss pattern its
name promises (the same assertions as tests/test_runner_up_miss_host.py), so that a fixture that stops provoking its
path fails here and not silently."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from tests import runner_up_miss as RM
from tests.util import assert_search_equal, product_from_oracle

pytestmark = pytest.mark.gpu


def run(index, orc, qs, ef, what):
    with H.kernel_log() as log:
        got = index.search_batch(qs, RM.TOPN, ef)
    assert any(k.startswith("hx_lean_f32_kernel<100,") for k in log), (what, dict(log))
    assert_search_equal(got, orc.search_batch(qs, RM.TOPN, ef, nthreads=8), what)


@pytest.fixture(scope="module")
def built():
    orc, vs, lv, qs = RM.built()
    return product_from_oracle(orc, vs, lv), orc, qs


@pytest.mark.parametrize("ef", RM.EFS)
def test_built_index(built, ef):
    index, orc, qs = built
    run(index, orc, qs, ef, "built ef=%d" % ef)


_INDEX = {}


@pytest.mark.parametrize("name,ef", RM.CASES)
def test_handmade_graph(name, ef):
    orc, rows, lv, qs, g = RM.handmade(name)
    adj0 = {i: g.adj[i] for i in range(RM.N)}
    _, _, passes = RM.replay(orc, adj0, qs[0], ef)
    RM.assert_pattern(name, ef, g, passes, orc.distance_batch(qs[0], np.arange(RM.N, dtype=np.uint32)))
    if name not in _INDEX:
        _INDEX[name] = product_from_oracle(orc, rows, lv)
    run(_INDEX[name], orc, qs, ef, "%s ef=%d" % (name, ef))
