"""The lean kernels' upper-layer walk against the CPU oracle of the same vector kind, through the C ABI: ids, distance
bits, counts and the three counters, at ef 10 and 64 (one list register) and 68 (head + tail), f32 and quant8 rows at
d = 100.  The f32 kernels request the front of the walk ahead (search_lean.hip); hx_lean_q8_kernel keeps the
walk that loads a row when it expands it (the same step was measured there and not merged) and is held to
the same cases.  The fixtures are tests/upper_walk.py's; every hand-made case first proves on the CPU replay that it has
the pattern its name promises (the assertions of tests/test_upper_walk_host.py; the pools of a case are ranked by its
kind's own distances), so that a fixture that stops provoking its path fails here and not silently."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import numeric_range as NR
from tests import upper_walk as UW
from tests.util import assert_search_equal, oracle_from_product

pytestmark = pytest.mark.gpu

LIST_OF = {10: "Lst<1>", 64: "Lst<1>", 68: "LstHT"}


KINDS = (UW.F32, UW.QUANT8)
KIND_ID = {UW.F32: "f32", UW.QUANT8: "quant8"}.get


def lean_kernel(ef, kind=UW.F32):
    lst = LIST_OF[ef]
    if kind == UW.QUANT8:
        return "hx_lean_q8_kernel<%s>" % (lst + " " if lst.endswith(">") else lst)
    return "hx_lean_f32_kernel<100, %s, 4>" % lst


def run(index, orc, qs, ef, what, kind=UW.F32):
    with H.kernel_log() as log:
        got = index.search_batch(qs, UW.TOPN, ef)
    assert lean_kernel(ef, kind) in log, (what, dict(log))
    assert_search_equal(got, orc.search_batch(qs, UW.TOPN, ef, nthreads=8), what)


@pytest.mark.parametrize("ef", UW.EFS)
@pytest.mark.parametrize("name", sorted(UW.CASES))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_ID)
def test_handmade_upper_layers(kind, name, ef):
    UW.assert_pattern(name, kind)
    c, orc = UW.fixture(name, kind)
    run(UW.product(name, kind), orc, c.queries, ef, "%s %s ef=%d" % (KIND_ID(kind), name, ef), kind)


@pytest.mark.parametrize("ef", UW.EFS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_ID)
def test_level0_entry(kind, ef):
    """held to what the `misplaced` runner of tests/graph_shapes.py holds: the status where the oracle raises, counts 0,
    ids all ones -- for every query of the call.  (`level0_neighbour`, a layer-1 row that lists a node of level 0, is
    refused by the product's import: tests/test_upper_walk_host.py.)"""
    name = "level0_entry"
    UW.assert_refused(name, kind)
    c, _ = UW.fixture(name, kind)
    idx = UW.product(name, kind)
    E = H._lib.ERR_NODE_NOT_IN_GRAPH
    with NR.unchecked():
        idx.search_batch(c.queries, UW.TOPN, ef)  # (the first call uploads the snapshot)
    with NR.unchecked() as rcs, H.kernel_log() as log:
        ids, _, counts, stats = idx.search_batch(c.queries, UW.TOPN, ef)[:4]
    what = "%s %s ef=%d" % (KIND_ID(kind), name, ef)
    assert [rc for rc in rcs if rc] == [E], (what, rcs)
    assert lean_kernel(ef, kind) in log, (what, dict(log))
    assert (np.asarray(stats)[:, 3].astype(np.int32) == E).all(), (what, np.asarray(stats)[:, 3])
    assert (counts == 0).all() and (ids == O.UINT32_MAX).all(), (what, counts, ids[:2])


@pytest.fixture(scope="module", params=KINDS, ids=KIND_ID)
def built(request):
    kind = request.param
    vs = H.synth_rows(0, 0x5EED0001, 0, UW.N_BUILT, UW.D)
    qs = H.synth_rows(0, 0x5EED0002, 0, UW.NQ_BUILT, UW.D)
    lv = O.draw_levels(UW.N_BUILT, UW.M, 0x5EED0003)
    index = H.HNSW.new(UW.M, 32, UW.D, kind)
    index.insert_bulk_device(vs, 8, False, levels=lv)
    return index, oracle_from_product(index, vs, lv), qs, kind


@pytest.mark.parametrize("ef", (64, 68))
def test_built_index(built, ef):
    index, orc, qs, kind = built
    assert orc.nb_layers >= 3
    run(index, orc, qs, ef, "built %s ef=%d" % (KIND_ID(kind), ef), kind)
