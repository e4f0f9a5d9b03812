"""The recipes of tests/graph_shapes.py do what they claim (no GPU needed: the oracle and the product's host accessors
only), for both kinds and m = 16 and 24; the selection rule names every walk routine compiled into the library; and
import_layer refuses a row that holds its own node on both sides."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests import graph_shapes as GS
from tests import kernel_matrix as KM
from tests.kernel_matrix import F32, Q8

D = 100
FIXTURES = [(kind, D, m) for kind in (Q8, F32) for m in (16, 24)]
fixtures = pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: "%s-d%d-m%d" % ("q8" if f[0] == Q8 else "f32", f[1], f[2]))


def call(fx, ef=100, nq=4):
    return KM.Call(fx[0], fx[1], fx[2], 0, "batch", ef, ef, nq, "default", 0, (), ())


def same_graph(idx, orc):
    return all(np.array_equal(a, b) for l in range(orc.nb_layers)
               for a, b in zip(idx.get_layer(l).csr(), orc.layer_csr(l)))


def test_the_background_is_the_circulant_graph():
    adj = GS.background()
    assert len(adj) == GS.N and all(len(r) == 8 for r in adj.values())
    assert all(i in adj[j] for i, r in adj.items() for j in r)
    seen, todo = {0}, [0]
    while todo:
        for j in adj[todo.pop()]:
            if j not in seen:
                seen.add(j)
                todo.append(j)
    assert len(seen) == GS.N


@fixtures
def test_collide_rows_stay_inside_the_last_buckets(fx):
    idx, orc, rows, g = GS.fixture(*fx, "collide")
    s0, s1 = GS.strides(fx[2])
    C = set(g["C"])
    assert len(C) >= 40 and g["ep"] in C
    if fx[2] == 16:
        assert (GS.home_bucket(g["C"], 12) >= 1024 - 3).all()
    # the top bits nest: the last buckets of a table twice the size, the last of a quarter-size one
    assert (GS.home_bucket(g["C"], 13) >= 2048 - 2 * (1024 - GS.home_bucket(g["C"], 12).min())).all()
    assert (GS.home_bucket(g["C"], 10) >= 256 - 2).all()
    assert idx.nb_layers() == 2 and set(idx.get_layer(1).iter_nodes().tolist()) == C
    for c in C:
        r0, r1 = idx.get_layer(0).neighbors(c), idx.get_layer(1).neighbors(c)
        assert c not in r0 and c not in r1
        assert len(r0 & C) >= s0 - 1 and len(r0) == s0, (c, len(r0 & C))
        assert len(r1 & C) == s1 == len(r1), (c, len(r1))
    assert same_graph(idx, orc)
    # more ids of one bucket than it and its successors to the end of the table hold: an insert has to wrap
    assert len(C) > 4 * (1024 - GS.home_bucket(g["C"], 12).min())


@fixtures
def test_chain_is_walked_to_its_end(fx):
    idx, orc, rows, g = GS.fixture(*fx, "chain")
    Q = GS.queries(call(fx), rows, g)
    assert idx.nb_layers() == 3 and same_graph(idx, orc)
    ids, _, _, stats = orc.search_batch(Q[4:5], 10, 10)  # q*
    assert int(stats[0, 1]) >= 2 * GS.CHAIN, stats
    dd = orc.distance_batch(Q[4], np.array(g["chain"], dtype=np.uint32))
    assert (dd[1:] < dd[:-1]).all()
    assert idx.get_layer(2).nb_nodes() == GS.CHAIN and idx.get_layer(1).nb_nodes() == 2 * GS.CHAIN


@fixtures
def test_degrees_every_hub_has_its_class(fx):
    idx, orc, rows, g = GS.fixture(*fx, "degrees")
    s0, s1 = GS.strides(fx[2])
    assert same_graph(idx, orc)
    for l, s in ((0, s0), (1, s1)):
        assert [k for _, k in g["hubs"][l]] == [0, 1, s - 1, s, s + 1, s + 30, s + 31, s + 32, s + 62, s + 63, s + 64]
        for hub, k in g["hubs"][l]:
            assert idx.get_layer(l).degree(hub) == k, (l, hub, k)
    for l in (0, 1):  # symmetric, no self connection
        ids, offs, nbrs = idx.get_layer(l).csr()
        rows_ = {int(n): set(nbrs[int(offs[i]):int(offs[i + 1])].tolist()) for i, n in enumerate(ids)}
        assert all(a not in r and all(a in rows_[b] for b in r) for a, r in rows_.items())
    Q = GS.queries(call(fx, 10), rows, g)[4:]
    hubs = g["hubs"][1] + g["hubs"][0]
    assert Q.shape[0] == len(hubs)
    ids, _, _, stats = orc.search_batch(Q, 10, 10, nthreads=8)
    for qi, (hub, k) in enumerate(hubs):
        assert int(stats[qi, 2]) >= k, (hub, k, stats[qi])
        if k:  # the walk reaches the hub
            assert hub in ids[qi], (hub, k, ids[qi])


@fixtures
@pytest.mark.parametrize("ef", [10, 100])
def test_small_counts_are_the_rings(fx, ef):
    idx, orc, rows, g = GS.fixture(*fx, "small", ef)
    assert idx.nb_layers() == 16 and same_graph(idx, orc)
    assert sorted(g["heads"]) == sorted({1, 2, 9, 10, 11, ef - 1, ef, ef + 1})
    Q = GS.queries(call(fx, ef), rows, g)
    for c, head in g["heads"].items():
        assert idx.get_layer(0).degree(head) == (0 if c == 1 else 1 if c == 2 else 2)
        orc.set_ep(head)
        for n in (10, ef):
            ids, _, counts, _ = orc.search_batch(Q, n, ef)
            assert (counts == min(n, c)).all(), (c, n, counts)
            assert ((ids[:, :min(n, c)] >= head) & (ids[:, :min(n, c)] < head + c)).all()
    # the background holds no edge to a ring
    ids, offs, nbrs = idx.get_layer(0).csr()
    n_ring = sum(g["heads"])
    assert nbrs[int(offs[n_ring]):].min() >= n_ring and nbrs[:int(offs[n_ring])].max() < n_ring


@fixtures
def test_misplaced_entry_point_is_refused_by_the_reference(fx):
    """searcher.rs:45-50: the entry point's row is looked up on the top layer, where a node of level 0 is not; the
    filtered restatement walks its upper layers with the same search_layer and states the same"""
    idx, orc, rows, g = GS.fixture(*fx, "misplaced")
    assert g["levels"][g["ep"]] == 0 and idx.nb_layers() == 16 and int(idx.params.ep) == g["ep"] == orc.ep
    Q = GS.queries(call(fx, 10), rows, g)
    with pytest.raises(O.OracleError) as e:
        orc.search_batch(Q, 10, 10)
    assert e.value.code == -3
    from tests.test_gpu_filtered import restated
    with pytest.raises(KeyError, match="%d not in Graph" % g["ep"]):
        FR.graph(restated(idx, rows), Q[0], 10, 10, lambda i: True)


def test_the_selection_names_every_walk_routine():
    from tests.test_kernel_matrix_complete import compiled_kernels
    sel = GS.selection()
    walks = {k for k in compiled_kernels() if k.split("<")[0] in GS.WALK_FAMILIES}
    assert len(walks) > 100
    missing = sorted(k for k in walks if GS.routine_of(k) not in sel)
    assert not missing, missing
    for key, (kernels, c, v2l) in sel.items():
        assert [GS.routine_of(k) for k in kernels] == [key] and c.entry in GS.WALK_ENTRIES
        assert all(v.group == "visited2l" for v in v2l)
    # list widths are kept, row shapes are not
    assert GS.routine_of("hx_search_kernel<1, 25, 100, 2, false>") == ("hx_search_kernel", "1", "2", "false")
    assert GS.routine_of("hx_lean_f32_kernel<128, LstHT, 2>") == ("hx_lean_f32_kernel", "128", "LstHT", "2")
    entries = {c.entry for _, c in GS.TABLE}
    assert entries == {"batch", "filtered", "layer", "device"}
    ids = [GS.table_id(kc) for kc in GS.TABLE]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("kind", [Q8, F32], ids=["q8", "f32"])
def test_import_layer_refuses_a_self_connection(kind):
    """graph.rs:38-40: no graph of the reference holds one; nothing is imported by the refused call"""
    n, d = 6, 8
    rows = H.synth_rows(0, 5, 0, n, d)
    ids = np.arange(n, dtype=np.uint32)
    good = (ids, np.arange(n + 1, dtype=np.uint64), ((ids + 1) % n).astype(np.uint32))
    bad_nbrs = good[2].copy()
    bad_nbrs[4] = 4
    idx = H.HNSW.new(4, None, d, kind)
    idx.import_points(rows, np.zeros(n, dtype=np.uint8))
    idx.import_layer(0, *good)
    with pytest.raises(H.HnswError) as e:
        idx.import_layer(0, ids, good[1], bad_nbrs)
    assert e.value.code == H._lib.ERR_SELF_CONNECTION and "node 4" in str(e.value), e.value
    assert all(np.array_equal(a, b) for a, b in zip(idx.get_layer(0).csr(), good))
    orc = O.OracleHNSW(4, None, d, kind)
    orc.import_points(rows, np.zeros(n, dtype=np.uint8))
    with pytest.raises(O.OracleError) as e:
        orc.import_layer(0, ids, good[1], bad_nbrs)
    assert e.value.code == -5 and orc.nb_layers == 0
    orc.import_layer(0, *good)
    assert all(np.array_equal(a, b) for a, b in zip(orc.layer_csr(0), good))
