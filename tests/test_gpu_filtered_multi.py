"""hnsw_search_batch_filtered_multi on the MI355X: every query of a call under its own allow-list.  Each row is held,
bit for bit, to the CPU restatement (tests/filtered_restate.py) applied with that query's own allowed-predicate: ids,
distance bits, counts, counters (n_dist, n_exp, sum_deg) and the path."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import LIMIT, _import_graph, masks, restated
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

NONE = -1  # mask_of entry of a query without an allow-list


def predicates(index, mask_list, deleted=()):
    """mask_of entry -> (allowed(id), admissible ids): the mask AND NOT deleted; NONE: every id < len"""
    n_points, dele, cache = index.len(), set(int(i) for i in deleted), {}

    def get(g):
        if g not in cache:
            words, bits = H.pack_allow(np.ones(n_points, dtype=bool) if g == NONE else mask_list[g], n_points)
            f = FR.allowed_fn(words, bits, n_points)
            a_ids = np.array([i for i in FR.allowed_ids_of(words, bits, n_points) if i not in dele], dtype=np.int64)
            cache[g] = ((lambda i, f=f: f(i) and i not in dele), a_ids)
        return cache[g]
    return get


def compare_row(got, qi, want, n, what):
    ids, dists, counts, stats, paths = got
    w_ids, w_d, w_c = FR.padded(want, n)
    assert counts[qi] == w_c, (what, qi, paths[qi])
    assert np.array_equal(ids[qi], w_ids), (what, qi, paths[qi], ids[qi], w_ids)
    assert np.array_equal(dists[qi].view(np.uint32), w_d.view(np.uint32)), (what, qi)
    assert tuple(int(x) for x in stats[qi, :3]) == tuple(want["counters"]), (what, qi, stats[qi], want["counters"])


def check_rows(index, ridx, Q, n, ef, mask_list, mask_of, exact_max, got, deleted=(), Qr=None, what="", skip=()):
    """every row of a multi call against the restatement under its own predicate (tests/test_gpu_filtered.check, per
    query); `skip`: rows checked by the caller"""
    Qr = Q if Qr is None else Qr
    pred = predicates(index, mask_list, deleted)
    ids, dists, counts, stats, paths = got
    for qi in range(Q.shape[0]):
        if qi in skip:
            continue
        allowed, a_ids = pred(int(mask_of[qi]))
        w = (what, qi, int(mask_of[qi]))
        assert stats[qi, 3] == 0, w
        if a_ids.size <= exact_max:
            assert paths[qi] == 1, w
            want = FR.exact(ridx, Qr[qi], n, a_ids)
        else:
            g = FR.graph(ridx, Qr[qi], n, ef, allowed)
            if g["visited0"] > LIMIT:
                assert paths[qi] == 2, (w, g["visited0"])
            if g["visited0"] + g["maxdeg0"] <= LIMIT:
                assert paths[qi] == 0, (w, g["visited0"])
            want = g if paths[qi] == 0 else FR.exact(ridx, Qr[qi], n, a_ids)
        compare_row(got, qi, want, n, w)


def run_check(index, ridx, Q, n, ef, mask_list, mask_of, exact_max=-1, **kw):
    index.set_option("filter_exact_max", exact_max)
    got = index.search_batch_filtered_multi(Q, n, ef, mask_list, mask_of)
    check_rows(index, ridx, Q, n, ef, mask_list, mask_of, exact_max, got, **kw)
    return got


def dealt(nq, n_masks, none_at=()):
    mo = np.arange(nq) % n_masks
    mo[list(none_at)] = NONE
    return mo


def graph_kernels(log):
    return {k: v for k, v in log.items() if k.startswith("hx_filt_graph_kernel")}


@pytest.fixture(scope="module", params=[H.VEC_QUANT8, H.VEC_F32], ids=["quant8", "f32"])
def glove(request, testdata):
    store, queries = testdata
    lv = O.draw_levels(1000, 12, 1)
    index = H.HNSW.new(12, None, 50, request.param).insert_bulk(store, 1, False, levels=lv)
    return index, restated(index, store), queries


# ---- 1. the reference's test data: six masks in one call ---------------------------------------------------------
@pytest.mark.parametrize("exact_max", [-1, 50])
@pytest.mark.parametrize("n,ef", [(10, 64), (1, 1), (64, 100), (10, 256), (64, 10)])
def test_reference_test_data(glove, n, ef, exact_max):
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    mo = dealt(40, 6, none_at=(7, 19, 33))
    got = run_check(index, ridx, queries[:40], n, ef, mask_list, mo, exact_max, what="n=%d ef=%d" % (n, ef))
    # the masks allow 1000, 521, 107, 4, 1 and 0 ids (tests/test_filtered_multi_host.py counts them): "0.01", "one" and
    # "none" go exact under 50, the others and the unmasked rows go graph, none of them near the threshold
    want_exact = (exact_max == 50) & np.isin(mo, (3, 4, 5))
    assert np.array_equal(got[4] == 1, want_exact)
    assert (got[2][mo == 5] == 0).all()  # the empty mask: count 0 on either path


# ---- 2. every compiled form of the graph kernel reads a per-query mask pointer -----------------------------------
FORMS = {(H.VEC_F32, 100): "1, 25, 100", (H.VEC_F32, 128): "1, 32, 128", (H.VEC_F32, 37): "1, 0, 0",
         (H.VEC_QUANT8, 100): "0, 4, 100", (H.VEC_QUANT8, 37): "0, 0, 0"}


@pytest.mark.parametrize("kind,d,inline", [(H.VEC_F32, 100, -1), (H.VEC_QUANT8, 100, 0), (H.VEC_QUANT8, 100, 1),
                                           (H.VEC_F32, 128, -1), (H.VEC_F32, 37, -1), (H.VEC_QUANT8, 37, -1)])
def test_shapes(kind, d, inline):
    vs = rand_vectors(3000, d, 40 + d)
    qs = rand_vectors(30, d, 41 + d)
    index = H.HNSW.new(16, 64, d, kind).insert_bulk(vs, 4, False, levels=O.draw_levels(3000, 16, 2))
    index.set_option("inline_rows", inline)
    index.set_option("filter_exact_max", -1)
    ridx = restated(index, vs)
    mask_list = [m for _, m in masks(3000, d)]
    mo = dealt(30, 6, none_at=(4, 17))
    index.search_batch_filtered_multi(qs[:2], 10, 64, mask_list, mo[:2])  # (uploads the snapshot)
    for (n, ef), r in (((10, 64), 1), ((64, 128), 2), ((64, 256), 4)):
        with H.kernel_log() as log:
            got = index.search_batch_filtered_multi(qs, n, ef, mask_list, mo)
        assert set(graph_kernels(log)) == {"hx_filt_graph_kernel<%s, %d>" % (FORMS[kind, d], r)}, dict(log)
        assert "hx_filt_compact_kernel" not in log, dict(log)
        check_rows(index, ridx, qs, n, ef, mask_list, mo, -1, got, what="d=%d n=%d ef=%d" % (d, n, ef))
        assert (got[4] == 0).all()


# ---- 3. one launch of the graph kernel, not one per mask ------------------------------------------------------------
def test_one_graph_launch_and_one_compaction_per_referenced_mask(glove):
    index, ridx, queries = glove
    rng = np.random.default_rng(31)
    mask_list = [rng.random(1000) < 0.3 for _ in range(8)]
    Q = np.concatenate([queries, queries])[:64]
    assert Q.shape[0] == 64
    mo = dealt(64, 8)
    index.set_option("filter_exact_max", -1)
    index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)  # (uploads the snapshot)
    c0, m0 = index.stat("filtered_multi_calls"), index.stat("filtered_multi_masks")
    with H.kernel_log() as log:
        got = index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)
    assert list(graph_kernels(log).values()) == [1], dict(log)  # nothing overflows on 1000 points: no re-run either
    assert "hx_filt_compact_kernel" not in log and "hx_filt_merge_kernel" not in log, dict(log)
    assert (got[4] == 0).all()
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, -1, got, what="one launch")
    ninth = mask_list + [rng.random(1000) < 0.3]
    with H.kernel_log() as log9:
        got9 = index.search_batch_filtered_multi(Q, 10, 64, ninth, mo)
    assert dict(log9) == dict(log)
    assert all(np.array_equal(a, b) for a, b in zip(got, got9))
    assert index.stat("filtered_multi_calls") == c0 + 2 and index.stat("filtered_multi_masks") == m0 + 16

    index.set_option("filter_exact_max", 10 ** 9)
    index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)
    mo5 = mo.copy()
    mo5[mo5 >= 5] = 2  # five of the eight masks are referenced
    for ml, mof, referenced in ((mask_list, mo, 8), (ninth, mo, 8), (ninth, mo5, 5)):
        with H.kernel_log() as log:
            got = index.search_batch_filtered_multi(Q, 10, 64, ml, mof)
        assert not graph_kernels(log), dict(log)
        assert log["hx_filt_compact_kernel"] == referenced and log["hx_filt_merge_kernel"] == referenced, dict(log)
        assert (got[4] == 1).all()
        check_rows(index, ridx, Q, 10, 64, ml, mof, 10 ** 9, got, what="exact, %d referenced" % referenced)
    # a mixed plan: the graph path's queries of several masks still share the one launch
    sizes = [int(m.sum()) for m in mask_list]
    cut = sorted(sizes)[3]  # four masks at or below: exact; four above: graph
    index.set_option("filter_exact_max", cut)
    with H.kernel_log() as log:
        got = index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)
    n_exact = sum(s <= cut for s in sizes)
    assert 0 < n_exact < 8 and list(graph_kernels(log).values()) == [1] and log["hx_filt_compact_kernel"] == n_exact
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, cut, got, what="mixed plan")


# ---- 4. all three paths in one call ----------------------------------------------------------------------------------
def test_graph_exact_and_overflow_paths_in_one_call():
    n, d = 30000, 8
    vs = rand_vectors(n, d, 81)
    rng = np.random.default_rng(82)
    nbrs = rng.integers(0, n, size=(n, 12))
    rows = [set() for _ in range(n)]
    for i in range(n):
        for j in nbrs[i].tolist():
            if j != i:
                rows[i].add(j)
                rows[j].add(i)
    index = _import_graph(vs, H.VEC_F32, 8, rows)
    ridx = restated(index, vs)
    sparse = rng.random(n) < 0.0005  # (drawn in the order of test_visited_table_exhaustion_takes_the_exact_path)
    dense = rng.random(n) < 0.5
    assert int(sparse.sum()) == 16
    six = np.array([3, 77, 4096, 12345, 20000, 29999])
    mask_list = [dense, sparse, six]
    qs = rand_vectors(8, d, 83)
    Q = np.repeat(qs, 4, axis=0)
    mo = np.tile(np.array([0, 1, 2, NONE]), 8)
    index.set_option("filter_exact_max", 10)
    index.search_batch_filtered_multi(Q[:1], 10, 64, mask_list, mo[:1])  # (uploads the snapshot)
    before = {k: index.stat(k) for k in ("filtered_overflow_exact", "filtered_queries_exact", "filtered_queries_graph",
                                         "filtered_multi_calls", "filtered_multi_masks")}
    got = index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)
    paths = got[4]
    assert np.array_equal(paths, np.tile(np.array([0, 2, 1, 0], dtype=np.uint8), 8)), paths
    after = {k: index.stat(k) for k in before}
    assert {k: after[k] - before[k] for k in before} == {
        "filtered_overflow_exact": 8, "filtered_queries_exact": 8, "filtered_queries_graph": 16,
        "filtered_multi_calls": 1, "filtered_multi_masks": 4}
    # dense, the six ids and the unmasked rows against the restatement; the sparse rows: the walk of the first two
    # restated to see that it fills the largest table, all eight against the exact restatement under `sparse`
    sparse_rows = [qi for qi in range(32) if mo[qi] == 1]
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, 10, got, what="three paths", skip=sparse_rows)
    allowed, a_ids = predicates(index, mask_list)(1)
    assert a_ids.size == 16
    for qi in sparse_rows[:2]:
        assert FR.graph(ridx, Q[qi], 10, 64, allowed)["visited0"] > LIMIT
    for qi in sparse_rows:
        assert got[3][qi, 3] == 0
        compare_row(got, qi, FR.exact(ridx, Q[qi], 10, a_ids), 10, ("sparse", qi))


# ---- 5. deletions compose ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8])
def test_deleted_ids_are_taken_out_of_every_mask(kind):
    n, d = 2000, 32
    vs = rand_vectors(n, d, 51)
    qs = rand_vectors(24, d, 52)
    index = H.HNSW.new(12, 48, d, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 12, 5))
    ridx = restated(index, vs)
    index.search_batch(qs[:1], 10, 64)
    uploads = index.stat("uploads")
    rng = np.random.default_rng(53)
    deleted = rng.choice(n, n // 10, replace=False)
    index.mark_deleted(deleted)
    mask_list = [rng.random(n) < 0.5, rng.random(n) < 0.1, np.sort(rng.choice(n, 40, replace=False)),
                 np.ones(n, dtype=bool)]
    mo = dealt(24, 4, none_at=(1, 10, 15, 20))
    for exact_max in (-1, 300):  # 300: the 0.1 mask and the 40 ids go exact
        got = run_check(index, ridx, qs, 10, 64, mask_list, mo, exact_max, deleted=deleted, what="deleted %d" % exact_max)
        assert not np.isin(got[0], deleted).any()
        if exact_max == 300:
            assert np.array_equal(got[4] == 1, np.isin(mo, (1, 2)))
    index.set_option("filter_exact_max", -1)
    got = index.search_batch_filtered_multi(qs, 10, 64, mask_list, mo)
    u_ids, u_d, u_c, u_s = index.search_batch(qs, 10, 64)  # the unfiltered entry under the same deletions
    none = mo == NONE
    assert np.array_equal(got[0][none], u_ids[none]) and np.array_equal(got[2][none], u_c[none])
    assert np.array_equal(got[1][none].view(np.uint32), u_d[none].view(np.uint32))
    assert np.array_equal(got[3][none], u_s[none])
    assert index.stat("uploads") == uploads


# ---- 6. the contract as written: each row is the single-mask call of its query -----------------------------------
@pytest.mark.parametrize("exact_max", [-1, 50])
def test_rows_equal_the_single_mask_entry(glove, exact_max):
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    mo = dealt(40, 6, none_at=(2, 21))
    Q = queries[:40]
    index.set_option("filter_exact_max", exact_max)
    for n, ef in ((10, 64), (64, 128)):
        got = index.search_batch_filtered_multi(Q, n, ef, mask_list, mo)
        for g in sorted(set(mo.tolist())):
            rows = np.flatnonzero(mo == g)
            one = index.search_batch_filtered(Q[rows], n, ef, np.ones(1000, dtype=bool) if g == NONE else mask_list[g])
            for a, b in zip(got, one):
                a = a[rows]
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b), (g, n, ef)


# ---- 7. after insert_vec patched the snapshot -----------------------------------------------------------------------
def test_after_insert_vec_patched_the_snapshot():
    d = 24
    vs = rand_vectors(1500, d, 61)
    index = H.HNSW.new(8, 32, d, H.VEC_QUANT8).insert_bulk(vs, 2, False, levels=O.draw_levels(1500, 8, 3))
    index.upload()
    new = rand_vectors(40, d, 62)
    for v in new:
        index.insert_vec(v, level=0)
    assert index.stat("point_patches") == 40 and index.stat("patch_fallbacks") == 0
    allv = np.concatenate([vs, new])
    ridx = restated(index, allv)
    rng = np.random.default_rng(64)
    # masks made before the inserts: 1500 bits, fewer than the index now holds
    mask_list = [np.ones(1500, dtype=bool), rng.random(1500) < 0.2]
    qs = np.concatenate([new[:8], rand_vectors(10, d, 63)])
    mo = dealt(18, 2, none_at=(0, 3, 5, 6, 11, 16))
    for exact_max in (-1, 400):
        got = run_check(index, ridx, qs, 10, 32, mask_list, mo, exact_max, what="patched")
        masked = mo != NONE
        found = got[0][masked]
        assert (found[found != _lib.UINT32_MAX] < 1500).all()     # the old masks leave the new points out
        free = got[0][~masked]
        assert ((free >= 1500) & (free != _lib.UINT32_MAX)).any()  # ... the unmasked rows can return them
    assert index.stat("point_patches") == 40 and index.stat("patch_fallbacks") == 0


# ---- 8. the cosine option; a NaN query in one group --------------------------------------------------------------
def test_cosine_option():
    d = 32
    vs = rand_vectors(2000, d, 91) - np.float32(0.5)
    qs = rand_vectors(20, d, 92) - np.float32(0.5)
    index = H.HNSW.new(12, 48, d, H.VEC_F32)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 2, False, levels=O.draw_levels(2000, 12, 4))

    def unit(x):
        s = np.zeros(x.shape[0], dtype=np.float32)
        for e in range(x.shape[1]):
            s = s + x[:, e] * x[:, e]
        return x / np.sqrt(s)[:, None]

    stored = np.stack([index.get_point(i).get_vals() for i in range(2000)])
    ridx = restated(index, stored)
    rng = np.random.default_rng(93)
    mask_list = [rng.random(2000) < 0.3, rng.random(2000) < 0.05, rng.random(2000) < 0.6]
    mo = dealt(20, 3, none_at=(5, 12))
    run_check(index, ridx, qs, 10, 64, mask_list, mo, -1, what="cosine graph", Qr=unit(qs))
    run_check(index, ridx, qs, 10, 64, mask_list, mo, 300, what="cosine mixed", Qr=unit(qs))


def raw_multi(index, Q, n, ef, mask_list, mask_of):
    """the C entry itself -> status and the five arrays (the Python mirror raises on a per-query error)"""
    words, bits = H.pack_allow_many(mask_list, index.len())
    mo = np.where(np.asarray(mask_of) < 0, H.MASK_NONE, mask_of).astype(np.uint32)
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    ids = np.full((nq, n), _lib.UINT32_MAX, dtype=np.uint32)
    dists = np.full((nq, n), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    stats = np.zeros((nq, 4), dtype=np.int32)
    paths = np.zeros(nq, dtype=np.uint8)

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    rc = _lib.lib().hnsw_search_batch_filtered_multi(
        index._h, p(Q, C.c_float), nq, n, ef, p(words, C.c_uint64), words.shape[0], bits, p(mo, C.c_uint32),
        p(ids, C.c_uint32), p(dists, C.c_float), p(counts, C.c_uint32),
        C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)), p(paths, C.c_uint8))
    return rc, (ids, dists, counts, stats.astype(np.int64), paths)


@pytest.mark.parametrize("exact_max", [-1, 50])
def test_a_nan_query_is_its_own_error(glove, exact_max):
    index, ridx, queries = glove
    mask_list = [m for _, m in masks(1000, 5)]
    mo = dealt(24, 6, none_at=(8,))
    Q = queries[:24].copy()
    Q[9, 4] = np.nan   # a query of "0.01": the graph path under -1, the exact path under 50
    Q[20, 0] = np.nan  # a query of "0.1": the graph path under both
    assert mo[9] == 3 and mo[20] == 2
    index.set_option("filter_exact_max", exact_max)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo)
    assert e.value.code == _lib.ERR_NAN_INPUT
    rc, got = raw_multi(index, Q, 10, 64, mask_list, mo)
    assert rc == _lib.ERR_NAN_INPUT
    for qi in (9, 20):
        assert got[3][qi, 3] == _lib.ERR_NAN_INPUT and got[2][qi] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
    check_rows(index, ridx, Q, 10, 64, mask_list, mo, exact_max, got, what="nan", skip=(9, 20))
