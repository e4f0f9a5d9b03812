"""The CPU restatement of the on-device build (oracle/batched_build.cpp) on its own, without a GPU: below the seed
size it is the reference's sequential build, its result does not depend on its threads, its graphs are valid HNSW
graphs, and the batch schedule is live.  tests/test_gpu_build_restatement.py holds the device build to it."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests.util import rand_vectors


def graph(orc):
    return orc.ep, orc.nb_layers, [tuple(a.tobytes() for a in orc.layer_csr(l)) for l in range(orc.nb_layers)]


def restated(vs, lv, m, ef_cons=32, kind=O.VEC_QUANT8, base=0, **kw):
    orc = O.OracleHNSW(m, ef_cons, vs.shape[1], kind)
    if base:
        orc.insert_bulk(vs[:base], lv[:base])
    st = orc.insert_bulk_batched(vs[base:], lv[base:], **kw)
    return orc, st


@pytest.mark.parametrize("kind,n,d,m", [(O.VEC_QUANT8, 2000, 24, 8), (O.VEC_F32, 2049, 17, 5), (O.VEC_QUANT8, 700, 50, 12)])
def test_below_the_seed_size_it_is_the_sequential_build(kind, n, d, m):
    """n <= 2048 (2049 with the entry point, which is not inserted): every point is the seed"""
    vs = rand_vectors(n, d, 11 + m)
    lv = O.draw_levels(n, m, 5 + m)
    orc, st = restated(vs, lv, m, kind=kind)
    assert st["batches"] == 0 and st["seed_points"] == n - 1
    assert graph(orc) == graph(O.OracleHNSW(m, 32, d, kind).insert_bulk(vs, lv))


def test_extension_below_the_seed_size_is_the_sequential_build():
    vs = rand_vectors(1500, 20, 3)
    lv = O.draw_levels(1500, 8, 4)
    lv[600:] = np.minimum(lv[600:], lv[:600].max())
    orc, st = restated(vs, lv, 8, base=600)
    want = O.OracleHNSW(8, 32, 20).insert_bulk(vs[:600], lv[:600]).insert_bulk(vs[600:], lv[600:])
    assert st["batches"] == 0 and graph(orc) == graph(want)


@pytest.mark.parametrize("kind", [O.VEC_QUANT8, O.VEC_F32])
def test_result_does_not_depend_on_the_threads(kind):
    vs = rand_vectors(6000, 16, 21)
    lv = O.draw_levels(6000, 8, 22)
    a, sa = restated(vs, lv, 8, kind=kind, nthreads=1)
    b, sb = restated(vs, lv, 8, kind=kind, nthreads=8)
    assert sa == sb and sa["batches"] > 0
    assert graph(a) == graph(b)


def assert_valid(orc, n, lv, kept_last_edges):
    """the invariants the GPU tests check on the device build: symmetric, no self-loops, no isolated node, every
    node on the layers up to its level, and rows past the cap only by the kept-last-edges mirrored after the build"""
    assert len(orc) == n
    over = 0
    for l in range(orc.nb_layers):
        ids, offs, nbrs = orc.layer_csr(l)
        assert np.array_equal(ids, np.flatnonzero(lv >= l).astype(np.uint32)), l
        adj = {int(i): set(nbrs[int(offs[k]):int(offs[k + 1])].tolist()) for k, i in enumerate(ids)}
        cap = orc.layer_m(l)
        for i, row in adj.items():
            assert i not in row
            assert len(ids) == 1 or row, "node %d isolated on layer %d" % (i, l)
            over += max(0, len(row) - cap)
            for nb in row:
                assert i in adj[nb], "edge %d-%d is one-way on layer %d" % (i, nb, l)
    assert over <= kept_last_edges, (over, kept_last_edges)


@pytest.mark.parametrize("m,base", [(8, 0), (5, 0), (8, 3000)], ids=["m8", "m5", "m8-extension"])
def test_graphs_are_valid(m, base):
    n = 7000
    vs = rand_vectors(n, 16, 31 + m)
    lv = O.draw_levels(n, m, 32 + m)
    if base:
        lv[base:] = np.minimum(lv[base:], lv[:base].max())
    orc, st = restated(vs, lv, m, base=base, batch_max=1024, batch_div=4)
    assert st["batches"] > 0 and st["seed_points"] == (0 if base else 2048)
    if m == 5:  # the seed leaves rows over the cap of 10 / 5: the clamp restores, phase 3 refuses
        assert 0 < st["clamp_restores"] < st["kept_last_edges"], st
    assert_valid(orc, n, lv, st["kept_last_edges"])


def test_batching_is_live():
    """schedules (8192, 8) and (64, 64) batch the same points differently, and the points of a batch do not see
    one another: the graphs differ (both valid)"""
    vs = rand_vectors(7000, 16, 41)
    lv = O.draw_levels(7000, 8, 42)
    a, sa = restated(vs, lv, 8, batch_max=8192, batch_div=8)
    b, sb = restated(vs, lv, 8, batch_max=64, batch_div=64)
    assert sa["batches"] < sb["batches"]
    assert sb["batches"] == -(-(7000 - 1 - 2048) // 64)
    assert graph(a) != graph(b)
    assert_valid(a, 7000, lv, sa["kept_last_edges"])
    assert_valid(b, 7000, lv, sb["kept_last_edges"])


def test_rejects_what_the_device_build_rejects():
    vs = rand_vectors(10, 8, 1)
    lv = np.zeros(10, np.uint8)
    with pytest.raises(O.OracleError):
        O.OracleHNSW(129, 32, 8).insert_bulk_batched(vs, lv)
    with pytest.raises(O.OracleError):
        O.OracleHNSW(8, 32, 8).insert_bulk_batched(vs, lv, batch_div=0)
