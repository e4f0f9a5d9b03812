"""Parity tests proper: the HIP search path (through the C ABI) against the CPU oracle on the same
index and queries.  Bar: ids bit-exact, distances bit-exact (tolerance stated by north_star: 1e-4),
traversal counters identical.  Every test here needs a real MI355X."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import (assert_search_equal, graph_difference, oracle_from_product, product_from_oracle,
                        rand_vectors)

pytestmark = pytest.mark.gpu


def both(vectors, levels, m, kind=H.VEC_QUANT8, threads=1, ef_cons=None):
    d = vectors.shape[1]
    index = H.HNSW.new(m, ef_cons, d, kind).insert_bulk(vectors, threads, False, levels=levels)
    return index, oracle_from_product(index, vectors, levels)


@pytest.fixture(scope="module")
def glove(testdata):
    store, queries = testdata
    lv = O.draw_levels(1000, 12, 1)
    index, orc = both(store, lv, 12)
    return index, orc, queries


@pytest.mark.parametrize("ef", [1, 5, 10, 64, 100])
def test_search_matches_oracle_on_reference_test_data(glove, ef):
    index, orc, queries = glove
    got = index.search_batch(queries, 10, ef)
    want = orc.search_batch(queries, 10, ef)
    assert_search_equal(got, want, "ef=%d" % ef)


def test_ann_by_vector_single_query_api(glove):
    index, orc, queries = glove
    for q in queries[:5]:
        assert index.ann_by_vector(q, 10, 100) == [int(x) for x in orc.ann_by_vector(q, 10, 100)]
    # ef < n returns fewer than n ids; ef = 0 behaves like ef = 1
    assert index.ann_by_vector(queries[0], 10, 3) == [int(x) for x in orc.ann_by_vector(queries[0], 10, 3)]
    assert len(index.ann_by_vector(queries[0], 10, 3)) == 3
    assert index.ann_by_vector(queries[0], 10, 0) == [int(x) for x in orc.ann_by_vector(queries[0], 10, 0)]
    assert index.ann_by_vector(queries[0], 0, 10) == []


def test_hnsw_glove_build_eval(glove):
    """hnsw/src/template.rs:518-572 end to end on the GPU: recall@10 > 0.99 at M = 12, ef = 100
    against brute force over the same quantised distances, and min degree > 0 on every layer."""
    index, orc, queries = glove
    bf_ids, bf_d = index.brute_force(queries, 10)
    o_ids, o_d = orc.brute_force(queries, 10)
    assert np.array_equal(bf_ids, o_ids) and np.array_equal(bf_d.view(np.uint32), o_d.view(np.uint32))
    ids, _, _, _ = index.search_batch(queries, 10, 100)
    hits = sum(len(set(a) & set(b)) for a, b in zip(ids, bf_ids))
    assert hits / (len(queries) * 10) > 0.99
    for layer in index.iter_layers():
        if layer.nb_nodes() > 1:
            assert min(layer.degree(n) for n in layer.iter_nodes()) > 0


def test_distance_batch_is_bit_exact(glove):
    index, orc, queries = glove
    ids = np.arange(1000, dtype=np.uint32)[::-1].copy()
    for q in queries[:4]:
        got, want = index.distance_batch(q, ids), orc.distance_batch(q, ids)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_search_layer_seam(glove):
    index, orc, queries = glove
    for layer, entries, ef in [(0, [3], 10), (0, [5, 700, 42], 24), (1, [int(orc.layer_nodes(1)[0])], 1),
                               (1, [int(x) for x in orc.layer_nodes(1)[:3]], 4)]:
        for q in queries[:6]:
            g_ids, g_d, g_s = index.search_layer(layer, q, entries, ef)
            w_ids, w_d, w_s = orc.search_layer(layer, q, entries, ef)
            assert np.array_equal(g_ids, w_ids)
            assert np.array_equal(g_d.view(np.uint32), w_d.view(np.uint32))
            assert tuple(int(x) for x in g_s) == tuple(int(x) for x in w_s)


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
@pytest.mark.parametrize("d", [1, 7, 10, 16, 33, 50, 64, 100, 128, 200, 256, 300, 600, 1030])
def test_dimensions_and_vector_kinds(kind, d):
    n, m = 600, 8
    vs = rand_vectors(n, d, 100 + d) * np.float32(2.0) - np.float32(0.5)
    qs = rand_vectors(40, d, 200 + d) * np.float32(2.0) - np.float32(0.5)
    index, orc = both(vs, O.draw_levels(n, m, d), m, kind)
    for ef in (1, 17, 64):
        assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef),
                            "kind=%d d=%d ef=%d" % (kind, d, ef))
    ids = np.arange(n, dtype=np.uint32)
    got, want = index.distance_batch(qs[0], ids), orc.distance_batch(qs[0], ids)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
@pytest.mark.parametrize("ef", [65, 128, 200, 300, 512, 513, 700, 1024])
def test_large_ef_uses_wider_lists(ef, kind):
    """two, four, eight list registers per lane; beyond 512 the any-dimension kernel with sixteen (ef <= 1024)"""
    n, d, m = 3000, 24, 16
    vs, qs = rand_vectors(n, d, 1), rand_vectors(32, d, 2)
    index, orc = both(vs, O.draw_levels(n, m, 9), m, kind=kind, threads=4)
    assert_search_equal(index.search_batch(qs, 100, ef), orc.search_batch(qs, 100, ef), "ef=%d" % ef)


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_ef_beyond_the_register_list_is_still_exact(kind):
    """ann_by_vector has no limit on ef (template.rs:306-311).  Above 1024 the list and the visited set live in
    HBM scratch (hx_search_spill_kernel): ids, distances and counters are still the oracle's, including ef
    larger than the index, n in the thousands, the search_layer seam, and a visited table that starts too
    small and is doubled by the host"""
    n, d, m = 5000, 100, 16
    vs, qs = rand_vectors(n, d, 21), rand_vectors(24, d, 22)
    index, orc = both(vs, O.draw_levels(n, m, 23), m, kind=kind, threads=4)
    for ef, k in ((1025, 10), (1500, 1200), (4096, 4096), (6000, 50)):
        assert_search_equal(index.search_batch(qs, k, ef), orc.search_batch(qs, k, ef), "ef=%d n=%d" % (ef, k))
    ids = index.ann_by_vector(qs[0], 10, 2048)  # the one-query entry of the reference's API
    assert ids == [int(x) for x in orc.search_batch(qs[:1], 10, 2048)[0][0]]
    # device-resident entry + finish
    import torch
    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(qs).to(dev)
    nq, k, ef = qs.shape[0], 20, 1300
    d_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d_c = torch.empty(nq, dtype=torch.int32, device=dev)
    d_s = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    index.search_batch_device(dQ.data_ptr(), nq, k, ef, d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), 0)
    index.search_batch_device_finish(dQ.data_ptr(), nq, k, ef, d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), 0)
    w_ids, w_d, _, _ = orc.search_batch(qs, k, ef)
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), w_ids) and np.array_equal(d_d.cpu().numpy(), w_d)


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_ef_above_512_at_the_specialised_dimensions(kind):
    """d = 100 normally runs the lean / specialised kernels; ef 600 and 1000 route it through the
    any-dimension kernel, n = 600 results per query"""
    n, d, m = 4000, 100, 16
    vs, qs = rand_vectors(n, d, 5), rand_vectors(16, d, 6)
    index, orc = both(vs, O.draw_levels(n, m, 11), m, kind=kind, threads=4)
    for ef in (600, 1000):
        assert_search_equal(index.search_batch(qs, 600, ef), orc.search_batch(qs, 600, ef), "ef=%d" % ef)


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_rows_longer_than_the_adjacency_stride(kind):
    """degree > stride happens; such rows spill into the overflow CSR -- also when the row
    belongs to the runner-up that the f32 loop evaluates speculatively"""
    n, d, m = 400, 12, 4  # layer-0 cap 8, stride 32
    vs, qs = rand_vectors(n, d, 3), rand_vectors(50, d, 4)
    lv = O.draw_levels(n, m, 3)
    orc = O.OracleHNSW(m, None, d, kind).insert_bulk(vs, lv)
    # graft 70 extra symmetric edges onto node 5 and 40 onto node 9 of layer 0
    ids, offs, nbrs = orc.layer_csr(0)
    adj = {int(i): set(int(x) for x in nbrs[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)}
    for hub, cnt in ((5, 70), (9, 40)):
        for t in range(100, 100 + cnt):
            adj[hub].add(t)
            adj[t].add(hub)
    rows = [sorted(adj[int(i)]) for i in ids]
    offs2 = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    nbrs2 = np.concatenate([np.array(r, dtype=np.uint32) for r in rows])
    orc2 = O.OracleHNSW(m, None, d, kind)
    orc2.import_points(vs, lv)
    orc2.import_layer(0, ids, offs2, nbrs2)
    for l in range(1, orc.nb_layers):
        orc2.import_layer(l, *orc.layer_csr(l))
    orc2.set_ep(orc.ep)
    index = product_from_oracle(orc2, vs, lv)
    assert index.get_layer(0).degree(5) > 64
    for inline_rows in (1, 0):
        index.set_option("inline_rows", inline_rows)
        for ef in (1, 10, 64):
            assert_search_equal(index.search_batch(qs, 10, ef), orc2.search_batch(qs, 10, ef),
                                "overflow ef=%d inline=%d" % (ef, inline_rows))


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_duplicate_and_constant_vectors(kind):
    """ties are broken by id (dist.rs:30-38); constant vectors quantise through a NaN (Q2)"""
    d = 20
    base = rand_vectors(50, d, 8)
    vs = np.concatenate([base, base, np.full((10, d), 0.25, np.float32), base[:20]])
    lv = O.draw_levels(len(vs), 6, 4)
    index, orc = both(vs, lv, 6, kind=kind)
    qs = np.concatenate([base[:20], np.full((2, d), 0.25, np.float32), rand_vectors(10, d, 9)])
    for ef in (1, 8, 40):
        assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef), "ties ef=%d" % ef)


def test_nan_query_is_an_error_not_a_result(glove):
    index, _, queries = glove
    q = queries[:3].copy()
    q[1, 7] = np.nan
    with pytest.raises(H.HnswError) as e:
        index.search_batch(q, 10, 64)
    assert e.value.code == _lib.ERR_NAN_INPUT


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_tiny_indexes(kind):
    for n in (1, 2, 3, 40):
        vs = rand_vectors(n, 9, n)
        lv = O.draw_levels(n, 4, n)
        index, orc = both(vs, lv, 4, kind=kind)
        qs = rand_vectors(5, 9, 77)
        assert_search_equal(index.search_batch(qs, 10, 16), orc.search_batch(qs, 10, 16), "n=%d" % n)
    with pytest.raises(H.HnswError):
        H.HNSW.new(4, None, 9).ann_by_vector(rand_vectors(1, 9, 1)[0], 1, 1)


def test_search_sees_later_inserts(glove, testdata):
    """the HBM snapshot is refreshed after a mutation (insert_vec after build, template.rs:478-490)"""
    store, queries = testdata
    lv = O.draw_levels(1000, 12, 1)
    index, orc = both(store[:500], lv[:500], 12)
    before = index.ann_by_vector(queries[0], 5, 50)
    assert before == [int(x) for x in orc.ann_by_vector(queries[0], 5, 50)]
    node = index.insert_vec(queries[0], level=0)
    assert index.ann_by_vector(queries[0], 1, 50) == [node]


@pytest.fixture(scope="module")
def synth20k():
    """the headline kernel variant: 100-d QUANT8, M = 16 (128-B vector rows, 128-B adjacency rows)"""
    n, d, m = 20000, 100, 16
    vs = H.synth_rows(0, 0x5EED0001, 0, n, d)
    qs = H.synth_rows(0, 0x5EED0002, 0, 256, d)
    lv = O.draw_levels(n, m, 0x5EED0003)
    index, orc = both(vs, lv, m, threads=8, ef_cons=32)
    return index, orc, qs


@pytest.mark.parametrize("inline_rows", [1, 0])
@pytest.mark.parametrize("ef", [16, 64, 96, 256])
def test_synthetic_glove_shaped_100d(synth20k, ef, inline_rows):
    """both HBM layouts of layer 0: inline rows (one coalesced block per expansion, next block
    prefetched) and compact rows + adjacency gather"""
    index, orc, qs = synth20k
    index.set_option("inline_rows", inline_rows)
    assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef, nthreads=8),
                        "ef=%d inline=%d" % (ef, inline_rows))
    index.set_option("inline_rows", -1)


@pytest.mark.parametrize("inline_rows", [1, 0])
def test_layouts_on_reference_test_data(glove, inline_rows):
    index, orc, queries = glove
    index.set_option("inline_rows", inline_rows)
    for ef in (1, 10, 100):
        assert_search_equal(index.search_batch(queries, 10, ef), orc.search_batch(queries, 10, ef),
                            "ef=%d inline=%d" % (ef, inline_rows))
    index.set_option("inline_rows", -1)


def test_true_recall_of_the_synthetic_set(synth20k):
    index, orc, qs = synth20k
    bf, _ = index.brute_force(qs[:64], 10)
    ids, _, _, _ = index.search_batch(qs[:64], 10, 64)
    hits = sum(len(set(a) & set(b)) for a, b in zip(ids, bf))
    assert hits / 640 > 0.97
    o_bf, _ = orc.brute_force(qs[:8], 10, nthreads=8)
    assert np.array_equal(bf[:8], o_bf)


def test_f32_kind_on_the_synthetic_set():
    n, d, m = 5000, 100, 16
    vs = H.synth_rows(1, 0x5EED0001, 0, n, d)
    qs = H.synth_rows(1, 0x5EED0002, 0, 64, d)
    index, orc = both(vs, O.draw_levels(n, m, 5), m, H.VEC_F32, threads=8, ef_cons=32)
    for ef in (10, 64):
        assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef, nthreads=8), "f32")


def test_device_pointer_entry_point(synth20k):
    """hnsw_search_batch_device: everything resident in HBM, launched on a torch stream"""
    import torch
    index, orc, qs = synth20k
    index.upload()
    nq, n, ef = qs.shape[0], 10, 64
    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(qs).to(dev)
    d_ids = torch.empty((nq, n), dtype=torch.int32, device=dev)
    d_dists = torch.empty((nq, n), dtype=torch.float32, device=dev)
    d_counts = torch.empty(nq, dtype=torch.int32, device=dev)
    d_stats = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        index.search_batch_device(dQ.data_ptr(), nq, n, ef, d_ids.data_ptr(), d_dists.data_ptr(),
                                  d_counts.data_ptr(), d_stats.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    w_ids, w_d, w_c, w_s = orc.search_batch(qs, n, ef, nthreads=8)
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), w_ids)
    assert np.array_equal(d_dists.cpu().numpy().view(np.uint32), w_d.view(np.uint32))
    st = d_stats.cpu().numpy()
    assert (st[:, 3] == 0).all() and np.array_equal(st[:, :3].astype(np.uint64), w_s)


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_device_pointer_entry_recovers_from_a_full_visited_table(kind):
    """a hub with 5000 neighbours fills the default 4096-slot visited table: the device entry flags the
    query (status OVERFLOW, never a row of made-up ids), hnsw_search_batch_device_finish re-runs it with a
    larger table and the answer is the oracle's"""
    import torch
    n, d, m = 9000, 100 if kind == H.VEC_F32 else 12, 4
    vs, qs = rand_vectors(n, d, 13), rand_vectors(24, d, 14)
    lv = O.draw_levels(n, m, 3)
    orc = O.OracleHNSW(m, None, d, kind).insert_bulk(vs, lv)
    ids, offs, nbrs = orc.layer_csr(0)
    adj = {int(i): set(int(x) for x in nbrs[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)}
    for t in range(100, 5100):
        adj[5].add(t)
        adj[t].add(5)
    rows = [sorted(adj[int(i)]) for i in ids]
    orc2 = O.OracleHNSW(m, None, d, kind)
    orc2.import_points(vs, lv)
    orc2.import_layer(0, ids, np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64),
                      np.concatenate([np.array(r, dtype=np.uint32) for r in rows]))
    for l in range(1, orc.nb_layers):
        orc2.import_layer(l, *orc.layer_csr(l))
    orc2.set_ep(orc.ep)
    index = product_from_oracle(orc2, vs, lv)
    index.upload()
    qs[0] = vs[5]  # this query certainly expands the hub
    nq, topn, ef = qs.shape[0], 10, 32
    dev = torch.device("cuda:0")
    dQ = torch.from_numpy(qs).to(dev)
    d_ids = torch.empty((nq, topn), dtype=torch.int32, device=dev)
    d_dists = torch.empty((nq, topn), dtype=torch.float32, device=dev)
    d_counts = torch.empty(nq, dtype=torch.int32, device=dev)
    d_stats = torch.empty((nq, 4), dtype=torch.int32, device=dev)
    args = (dQ.data_ptr(), nq, topn, ef, d_ids.data_ptr(), d_dists.data_ptr(), d_counts.data_ptr(), d_stats.data_ptr(), 0)
    index.search_batch_device(*args)
    torch.cuda.synchronize()
    st = d_stats.cpu().numpy()
    assert st[0, 3] == _lib.ERR_OVERFLOW, st[:3]
    assert (d_ids.cpu().numpy().view(np.uint32)[st[:, 3] != 0] == O.UINT32_MAX).all()
    index.search_batch_device_finish(*args)
    want = orc2.search_batch(qs, topn, ef)
    got = (d_ids.cpu().numpy().view(np.uint32), d_dists.cpu().numpy(), d_counts.cpu().numpy().view(np.uint32),
           d_stats.cpu().numpy().astype(np.int64))
    assert (got[3][:, 3] == 0).all()
    assert_search_equal(got, want, "after finish")
    # the host-pointer entry does the same by itself
    assert_search_equal(index.search_batch(qs, topn, ef), want, "host entry")
    # ... also on its copying branch (calls of more than 512 queries: the result block comes back by a D2H copy)
    reps = 512 // nq + 1
    tiled = np.ascontiguousarray(np.tile(qs, (reps, 1)))
    assert tiled.shape[0] > 512
    want_tiled = tuple(np.concatenate([np.asarray(w)] * reps) for w in want)
    assert_search_equal(index.search_batch(tiled, topn, ef), want_tiled, "host entry, copying branch")


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
@pytest.mark.parametrize("m", [24, 32, 48])
def test_wide_adjacency_rows(kind, m):
    """m > 16: layer-0 rows of 64 / 128 slots are walked in several passes"""
    n, d = 2500, 20
    vs, qs = rand_vectors(n, d, 300 + m), rand_vectors(48, d, 400 + m)
    index, orc = both(vs, O.draw_levels(n, m, m), m, kind, threads=4)
    assert max(index.get_layer(0).degree(i) for i in range(0, n, 7)) > 32
    for ef in (1, 40, 130):
        assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef, nthreads=4),
                            "m=%d kind=%d ef=%d" % (m, kind, ef))


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_bert_sized_vectors(kind):
    """d = 768 (BASELINE configs[2] dimension): the any-dimension distance path"""
    n, d, m = 400, 768, 8
    vs, qs = rand_vectors(n, d, 77), rand_vectors(16, d, 78)
    index, orc = both(vs, O.draw_levels(n, m, 5), m, kind)
    for ef in (1, 32):
        assert_search_equal(index.search_batch(qs, 10, ef), orc.search_batch(qs, 10, ef), "d=768 ef=%d" % ef)
    ids = np.arange(n, dtype=np.uint32)
    got, want = index.distance_batch(qs[0], ids), orc.distance_batch(qs[0], ids)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_pointer_search_is_reentrant(glove):
    """ann_by_vector takes &self in the reference (template.rs:306): concurrent callers on one handle;
    every call leases its own scratch and stream"""
    import threading
    index, orc, queries = glove
    want = orc.search_batch(queries, 10, 48)
    got, errs = [None] * 6, []

    def work(t):
        try:
            for _ in range(5):
                got[t] = index.search_batch(queries, 10, 48)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for t in range(6):
        assert_search_equal(got[t], want, "thread %d" % t)


def test_host_pointer_batch_api_matches_single_queries(glove):
    """hnsw_search_batch (nq queries) == nq calls of hnsw_search (the reference's one-query API)"""
    index, _, queries = glove
    ids, _, counts, _ = index.search_batch(queries[:12], 7, 30)
    for q, row, c in zip(queries[:12], ids, counts):
        assert index.ann_by_vector(q, 7, 30) == [int(x) for x in row[:c]]


# ---------------------------------------------------------------------------------------------------
# on-device build: judged by recall and graph invariants, not by identity
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_inputs():
    n, d, m = 30000, 100, 16
    vs = H.synth_rows(0, 0x5EED0001, 0, n, d)
    qs = H.synth_rows(0, 0x5EED0002, 0, 256, d)
    lv = O.draw_levels(n, m, 0x5EED0003)
    cpu = H.HNSW.new(m, 32, d).insert_bulk(vs, 8, False, levels=lv)
    return cpu, vs, qs, lv


# connect step on the host (1: the reference's make_connections / prune on CPU threads) or on the
# device (2: request / prune / remove kernels)
@pytest.fixture(scope="module", params=[1, 2], ids=["host-connect", "device-connect"])
def gpu_built(request, build_inputs):
    cpu, vs, qs, lv = build_inputs
    dev = H.HNSW.new(16, 32, 100)
    dev.set_option("gpu_build", request.param)
    with H.kernel_log() as log:
        dev.insert_bulk_device(vs, 8, False, levels=lv)
    dev.build_mode, dev.build_kernels = request.param, dict(log)
    return dev, cpu, vs, qs, lv


def test_device_build_makes_a_valid_graph(gpu_built):
    dev, _, vs, _, _ = gpu_built
    assert dev.len() == len(vs) and dev.assert_param_compliance()
    # host connect: the changed rows go back to HBM through the row scatter; device connect: the connect kernel
    want = "hx_scatter_rows_kernel" if dev.build_mode == 1 else "hx_connect_kernel<0, 100, 1>"
    assert want in dev.build_kernels and "hx_insert_kernel<0, 100>" in dev.build_kernels, dev.build_kernels
    for layer in dev.iter_layers():
        ids, offs, nbrs = layer.csr()
        adj = {int(i): set(int(x) for x in nbrs[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)}
        for i in list(adj)[::97]:
            assert i not in adj[i]
            for nb in adj[i]:
                assert i in adj[nb], "edge %d-%d is one-way on layer %d" % (i, nb, layer.level)
        if len(ids) > 1:
            assert min(len(s) for s in adj.values()) > 0


def test_device_build_recall_matches_the_cpu_build(gpu_built):
    dev, cpu, _, qs, _ = gpu_built
    truth, _ = cpu.brute_force(qs, 10)
    rec = {}
    for name, idx in (("device", dev), ("cpu", cpu)):
        ids, _, _, _ = idx.search_batch(qs, 10, 64)
        rec[name] = sum(len(set(a) & set(b)) for a, b in zip(ids.tolist(), truth.tolist())) / (len(qs) * 10)
    assert rec["device"] > 0.97 and rec["device"] > rec["cpu"] - 0.01, rec


def test_search_on_a_device_built_graph_is_still_exact(gpu_built):
    dev, _, vs, qs, lv = gpu_built
    orc = oracle_from_product(dev, vs, lv)
    assert_search_equal(dev.search_batch(qs, 10, 64), orc.search_batch(qs, 10, 64, nthreads=8), "device-built")


@pytest.mark.parametrize("mode", [1, 2])
def test_device_build_extends_an_existing_index(build_inputs, mode):
    _, vs, qs, lv = build_inputs
    idx = H.HNSW.new(16, 32, 100).insert_bulk(vs[:5000], 8, False, levels=lv[:5000])
    idx.set_option("gpu_build", mode)
    # a later point above the current top layer would become an entry point that is never connected
    # (the reference's own TODO, hnsw/src/template.rs:283-290): keep the levels below it
    lv2 = np.minimum(lv[5000:12000], lv[:5000].max())
    # host connect on one thread: racing threads may push a row of the tiny top layer past the 1.1 x
    # slack of assert_param_compliance, exactly like the reference's own multi-threaded build
    idx.insert_bulk(vs[5000:12000], 1 if mode == 1 else 8, False, levels=lv2)  # routed to the device build
    assert idx.len() == 12000 and idx.assert_param_compliance()
    truth, _ = idx.brute_force(qs[:64], 10)
    ids, _, _, _ = idx.search_batch(qs[:64], 10, 64)
    assert sum(len(set(a) & set(b)) for a, b in zip(ids.tolist(), truth.tolist())) / 640 > 0.97


@pytest.mark.parametrize("kind,m,d", [(H.VEC_F32, 8, 33), (H.VEC_QUANT8, 24, 64), (H.VEC_QUANT8, 5, 100),
                                      (H.VEC_QUANT8, 64, 100), (H.VEC_F32, 64, 48), (H.VEC_QUANT8, 128, 60),
                                      (H.VEC_F32, 128, 100)])
def test_device_connect_other_shapes(kind, m, d):
    """device connect on other row strides (m = 5 -> 16 slots, 24 -> 64 slots), the f32 kind, and the M = 64 and
    128 of the reference's own build benches (hnsw/benches/hnsw_benchmarks.rs:7): 128- and 256-slot layer-0 rows,
    two and four registers per lane in hx_connect_kernel / hx_remove_kernel, up to 128 selected per layer"""
    n = 12000 if m <= 32 else 8000
    vs = H.synth_rows(0, 0xC0FFEE + m, 0, n, d)
    qs = H.synth_rows(0, 0xBEEF + m, 0, 128, d)
    lv = O.draw_levels(n, m, 9)
    idx = H.HNSW.new(m, 48, d, kind)
    idx.set_option("gpu_build", 2)
    idx.insert_bulk_device(vs, 8, False, levels=lv)
    assert idx.len() == n
    # with caps as small as m = 5 one kept-last-edge already exceeds the 1.1 x slack of
    # assert_param_compliance (the CPU build of the same data does too): bound the degrees directly
    assert m < 8 or idx.assert_param_compliance()
    for layer in idx.iter_layers():
        ids, offs, nbrs = layer.csr()
        deg = np.diff(offs)
        assert deg.max() <= (2 * m if layer.level == 0 else m) + 2
        assert len(ids) == 1 or deg.min() >= 1
        adj = {int(i): set(int(x) for x in nbrs[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)}
        for i in list(adj)[::53]:
            assert i not in adj[i]
            for nb in adj[i]:
                assert i in adj[nb], "edge %d-%d is one-way on layer %d" % (i, nb, layer.level)
    truth, _ = idx.brute_force(qs, 10)
    ids, _, _, _ = idx.search_batch(qs, 10, 96)
    rec = sum(len(set(a) & set(b)) for a, b in zip(ids.tolist(), truth.tolist())) / (len(qs) * 10)
    assert rec > 0.95, rec
    if m > 32:  # recall equals the CPU build's (the reference's algorithm on the host threads)
        cpu = H.HNSW.new(m, 48, d, kind).insert_bulk(vs, 8, False, levels=lv)
        c_ids, _, _, _ = cpu.search_batch(qs, 10, 96)
        c_rec = sum(len(set(a) & set(b)) for a, b in zip(c_ids.tolist(), truth.tolist())) / (len(qs) * 10)
        assert rec >= c_rec - 0.01, (rec, c_rec)
    # and the search on it is still the reference's search
    orc = oracle_from_product(idx, vs, lv)
    assert_search_equal(idx.search_batch(qs, 10, 40), orc.search_batch(qs, 10, 40, nthreads=8), "device-connect")


# ---------------------------------------------------------------------------------------------------
# sharded on-device build (BASELINE configs[4]): two ranks, gloo rendezvous, both on this one GPU --
# the exchange is the only thing that differs from an 8-GPU run (RCCL there, host-staged gloo here)
# ---------------------------------------------------------------------------------------------------
def _sharded_build_worker(rank, world, port, outdir):
    import os
    import sys
    import torch.distributed as dist
    from tests.conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import hnsw_rs_amd as HH
    n, d, m = 20000, 100, 16
    vs = HH.synth_rows(0, 0x5EED0001, 0, n, d)
    lv = HH.draw_levels(m, n)
    idx = HH.HNSW.new(m, 32, d)
    with HH.kernel_log() as klog:
        idx.insert_bulk_sharded(vs, 4, False, levels=lv)
    np.save(os.path.join(outdir, "kernels%d.npy" % rank), np.array(sorted(klog)))
    out = {}
    for layer in idx.iter_layers():
        ids, offs, nbrs = layer.csr()
        # rows as sorted sets: the order inside a row is not part of the graph
        rows = [np.sort(nbrs[int(offs[k]):int(offs[k + 1])]) for k in range(len(ids))]
        out["ids%d" % layer.level] = ids
        out["offs%d" % layer.level] = offs
        out["nbrs%d" % layer.level] = np.concatenate(rows) if rows else nbrs
    qs = HH.synth_rows(0, 0x5EED0002, 0, 128, d)
    truth, _ = idx.brute_force(qs, 10)
    got, _, _, _ = idx.search_batch(qs, 10, 64)
    out["recall"] = np.array([sum(len(set(a) & set(b)) for a, b in zip(got.tolist(), truth.tolist())) / 1280.0])
    out["compliant"] = np.array([1 if idx.assert_param_compliance() else 0])
    # phases 2 / 3 by row ownership: what this rank changed as an owner, what it received from the others
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    np.save(os.path.join(outdir, "stats%d.npy" % rank),
            np.array([idx.stat("build_rows_owned"), idx.stat("build_rows_received"), idx.stat("build_exchange_bytes")]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_device_build_two_ranks(tmp_path, world):
    """world 3: the row owners (id % 3) and the position slices of a batch do not line up anywhere"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sharded_build_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = np.load(tmp_path / "rank0.npz")
    for r in range(1, world):
        r1 = np.load(tmp_path / ("rank%d.npz" % r))
        assert sorted(r0.files) == sorted(r1.files)
        for k in r0.files:  # identical replicas, edge for edge
            assert np.array_equal(r0[k], r1[k]), (r, k)
    assert r0["recall"][0] > 0.97 and r0["compliant"][0] == 1
    # every rank ran the sharded build's own kernels: record filter, row packing, row application
    for r in range(world):
        ks = set(np.load(tmp_path / ("kernels%d.npy" % r)).tolist())
        assert {"hx_filter_records_kernel", "hx_pack_rows_kernel", "hx_apply_rows_kernel"} <= ks, (r, ks)
    # every rank connected / pruned only the rows it owns and received the others: the rows owned sum to the rows
    # received by any one rank plus its own
    st = np.stack([np.load(tmp_path / ("stats%d.npy" % r)) for r in range(world)])
    assert (st[:, 0] > 0).all() and (st[:, 1] > 0).all() and (st[:, 2] > 0).all(), st
    assert all(int(st[:, 0].sum()) == int(st[r, 0] + st[r, 1]) for r in range(world)), st
    # and the same graph as the single-GPU on-device build of the same input: the sharding only
    # changes who runs which search, and the searches of a batch do not depend on each other
    n, d, m = 20000, 100, 16
    vs = H.synth_rows(0, 0x5EED0001, 0, n, d)
    one = H.HNSW.new(m, 32, d).insert_bulk_device(vs, 4, False, levels=H.draw_levels(m, n))
    for layer in one.iter_layers():
        ids, offs, nbrs = layer.csr()
        rows = [np.sort(nbrs[int(offs[k]):int(offs[k + 1])]) for k in range(len(ids))]
        assert np.array_equal(r0["offs%d" % layer.level], offs)
        assert np.array_equal(r0["nbrs%d" % layer.level], np.concatenate(rows))
    # which is the batch-synchronous build restated on the CPU, edge for edge (oracle/batched_build.cpp): that
    # pins the sharded builds transitively
    orc = O.OracleHNSW(m, 32, d)
    orc.insert_bulk_batched(vs, H.draw_levels(m, n), nthreads=8)
    diff = graph_difference(one, orc)
    assert diff is None, diff
