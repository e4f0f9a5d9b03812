"""Multi-vector search on the GPU (include/hnsw_mi355x.h, "multi-vector search"), held to the numpy restatement of the
fusion (hnsw_rs_amd.multi.fuse_lists; tests/test_multi_host.py holds that to a plain loop) over the CPU oracle's distances
(OracleHNSW.distance_batch) and search (OracleHNSW.search_batch).  All comparisons are exact: ids, score BITS, counts,
unique, counters and statuses.
  1. hnsw_fuse_lists_device alone over host-made lists at the pass boundaries of both vector kinds and the table's end:
     one launch and nothing else, guard words, no word unwritten, a bad id and a NaN vector failing their query alone;
  2. search_batch_multi against the fusion of the ORACLE's lists, T = 3 and T = 1;
  3. the entry point: deletions, the cosine option, a replica handle, launch accounting;
  4. capture and replay of the primitive and of the chain search -> fuse on a torch stream.
The indexes are those of tests/test_gpu_from_rows.py (built once, shared, left unchanged)."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import multi_cases as MC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import (M, N, SHAPES, capture_and_replay, guarded, kernel_of, unguard, up,  # noqa: F401
                                      world)
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
NQ = 64
T3, POOL, TOPN, EF = 3, 16, 10, 32
QUERY_SEED = 7  # (chosen on the CPU: the oracle's lists meet MC.exercised on all four shapes)
# candidate totals at the pass boundaries of both vector kinds (32 and 64 entries a pass) and at the table's end
TOTALS = {31: (1, 31), 32: (2, 16), 33: (3, 11), 63: (3, 21), 64: (4, 16), 65: (5, 13), 200: (8, 25), 256: (16, 16)}


def summed_stats(stats_in, statuses):
    """the T incoming records of a query as the fusion leaves them: wrapping sums, the fusion's status"""
    s = (np.asarray(stats_in).astype(np.uint64)[:, :, :3].sum(axis=1) & 0xFFFFFFFF).astype(np.int64)
    return np.concatenate([s, (np.asarray(statuses).astype(np.int64) & 0xFFFFFFFF)[:, None]], axis=1)


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def fuse_on_device(index, Q, w, mode, ids, counts, stats, n_out, extras=True):
    import torch
    nq, T, pool = ids.shape
    d_in = (up(Q), None if w is None else up(w), up(ids), None if counts is None else up(counts),
            None if stats is None else up(stats.astype(np.uint32)))
    sizes = {"ids": nq * n_out, "scores": nq * n_out, "counts": nq if extras else 0, "unique": nq if extras else 0,
             "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.fuse_lists_device(nq, T, pool, n_out, mode, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], out["ids"], out["scores"],
                                out["counts"], out["unique"], out["stats"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shape = (nq, n_out)
    return (got["ids"].reshape(shape), got["scores"].view(np.float32).reshape(shape), got["counts"], got["unique"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4).astype(np.int64)), log


def host_made_lists(stored, T, pool, seed):
    """NQ queries of T lists: ids drawn where the index holds every row twice (0 .. 99 and 1400 .. 1499: equal scores, the
    id decides) and anywhere, duplicates inside and across lists, ragged counts, a stats record per list; vectors near
    stored rows.  Planted: 0 no entry; 1 the T lists identical; 2 every entry distinct; 4 an id equal to the length; 5 a NaN vector; 6 a failed
    incoming status on its last vector.  -> Q, weights, ids, counts, stats [NQ, T, 4]"""
    rng = np.random.default_rng(seed)
    twins = np.concatenate([np.arange(100), np.arange(1400, 1500)])
    ids = np.where(rng.random((NQ, T, pool)) < 0.5, rng.choice(twins, (NQ, T, pool)), rng.integers(0, N, (NQ, T, pool)))
    ids = ids.astype(np.uint32)
    counts = rng.integers(0, pool + 1, (NQ, T)).astype(np.uint32)
    counts[::3] = pool
    counts[2] = pool + 5
    counts[0] = 0
    ids[1] = ids[1, 0][None, :]
    counts[1] = pool
    ids[2] = rng.permutation(N)[:T * pool].reshape(T, pool)  # all distinct: T * pool candidates, the kernel's last pass full
    ids[4, T - 1, 0], counts[4, T - 1] = N, pool
    stats = rng.integers(2 ** 31, 2 ** 32, (NQ, T, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    stats[6, T - 1, 3] = _lib.ERR_OVERFLOW & 0xFFFFFFFF
    Q = stored[rng.integers(0, N, (NQ, T))] + rng.normal(0, 0.05, (NQ, T, stored.shape[1])).astype(np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    Q[5, T - 1, stored.shape[1] // 2] = np.nan
    w = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0, 1.0, 2.0], dtype=np.float32), (NQ, T))
    return Q, np.ascontiguousarray(w), ids, counts, stats


@pytest.mark.parametrize("total", list(TOTALS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_primitive_alone_is_the_restatement_bit_for_bit(name, total):
    index, orc, stored = world(name)
    index.upload()
    T, pool = TOTALS[total]
    assert T * pool == total
    Q, w, ids, counts, stats = host_made_lists(stored, T, pool, 100 * total + len(name))
    statuses = stats[:, :, 3].astype(np.uint32).view(np.int32).astype(np.int64)
    launches = index.stat("multi_fuse_launches")
    # with everything: weights, counts, stats and every optional output
    for mode, n_out in ((H.FUSE_SUM, min(10, pool)), (H.FUSE_MIN, pool)):
        what = "%s total=%d mode=%d" % (name, total, mode)
        got, log = fuse_on_device(index, Q, w, mode, ids, counts, stats, n_out)
        assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
        want = H.fuse_lists(Q, w, mode, ids, counts, statuses, orc.distance_batch, n_out, N)
        MC.assert_fused_equal(got[:4], want, what)
        assert np.array_equal(got[4], summed_stats(stats, want[4])), what
        # a bad id, a NaN vector and a failed status fail their query alone
        assert want[4][4] == _lib.ERR_ARG and want[4][5] == _lib.ERR_NAN_INPUT and want[4][6] == _lib.ERR_OVERFLOW
        assert (want[4] != 0).sum() == 3 and want[2][0] == 0 and want[3][1] <= pool and want[3][2] == total
        for q in (4, 5, 6):
            assert got[2][q] == 0 and got[3][q] == 0 and (got[0][q] == MAX).all() and np.isposinf(got[1][q]).all()
        assert (got[2][[3, 9]] >= 1).all()  # (every third query has full counts)
    # bare: no weights, no counts (pads mark the absent entries), no stats, no optional output
    bare = ids.copy()
    bare[np.arange(pool)[None, None, :] >= counts[:, :, None]] = MAX
    bare[6] = MAX  # (without statuses query 6 cannot fail: it has no entry instead)
    got, log = fuse_on_device(index, Q, None, H.FUSE_SUM, bare, None, None, min(10, pool), extras=False)
    want = H.fuse_lists(Q, None, H.FUSE_SUM, bare, None, None, orc.distance_batch, min(10, pool), N)
    MC.assert_fused_equal((got[0], got[1]), want, name + " bare")
    assert got[2] is None and got[3] is None and got[4] is None and dict(log) == {kernel_of(index): 1}
    assert index.stat("multi_fuse_launches") == launches + 3


# ---- 2. the search against the fusion of the oracle's lists --------------------------------------------------------------
def oracle_lists(orc, Q, pool, ef):
    nq, T = Q.shape[:2]
    c = orc.search_batch(Q.reshape(nq * T, -1), pool, ef)
    stats = np.concatenate([np.asarray(c[3]).astype(np.int64), np.zeros((nq * T, 1), dtype=np.int64)], axis=1)
    return np.asarray(c[0]).reshape(nq, T, pool), np.asarray(c[1]).reshape(nq, T, pool), np.asarray(c[2]).reshape(nq, T), \
        stats.reshape(nq, T, 4)


@pytest.mark.parametrize("name", list(SHAPES))
def test_search_is_the_fusion_of_the_oracles_lists(name):
    index, orc, stored = world(name)
    Q = MC.near_far_queries(stored, T3, NQ, QUERY_SEED)
    c_ids, _, c_counts, c_stats = oracle_lists(orc, Q, POOL, EF)
    w = np.random.default_rng(3).choice(np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32), (NQ, T3))
    w[5, 1] = -1.0
    plain = H.fuse_lists(Q, None, "sum", c_ids, c_counts, None, orc.distance_batch, TOPN, N)
    overlap, spread, fill = MC.exercised(c_ids.reshape(NQ * T3, POOL), c_counts.reshape(-1), plain[0], T3, POOL, NQ)
    assert overlap, "no near query's lists overlap"
    assert spread, "no far query has more candidates than one list"
    assert fill, "no answer holds an id that one of its lists misses: the fill is not exercised"
    for mode in ("sum", "min"):
        for weights in (None, w):
            what = "%s mode=%s weights=%s" % (name, mode, weights is not None)
            want = H.fuse_lists(Q, weights, mode, c_ids, c_counts, None, orc.distance_batch, TOPN, N)
            got = index.search_batch_multi(Q, TOPN, POOL, EF, weights=weights, mode=mode)
            MC.assert_fused_equal(got[:4], want, what)
            assert np.array_equal(got[4], summed_stats(c_stats, want[4])), what
            assert (got[2] == TOPN).all() and (got[4][:, 3] == 0).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_vector_is_the_fusion_and_the_search_itself(name):
    index, orc, stored = world(name)
    Q = MC.near_far_queries(stored, 1, NQ, QUERY_SEED)
    c_ids, c_dists, c_counts, c_stats = oracle_lists(orc, Q, POOL, EF)
    want = H.fuse_lists(Q, None, "sum", c_ids, c_counts, None, orc.distance_batch, TOPN, N)
    got = index.search_batch_multi(Q, TOPN, POOL, EF)
    MC.assert_fused_equal(got[:4], want, name)
    assert np.array_equal(got[4], summed_stats(c_stats, want[4])) and (got[3] == POOL).all()
    # the search's own first n, where its order is decided by the distances alone
    clear = [q for q in range(NQ) if len(set(c_dists[q, 0].view(np.uint32).tolist())) == POOL]
    assert len(clear) >= 8, "too few lists without two equal distances"
    assert np.array_equal(got[0][clear], c_ids[clear, 0, :TOPN])
    assert np.array_equal(got[1][clear].view(np.uint32), np.ascontiguousarray(c_dists[clear, 0, :TOPN]).view(np.uint32))


# ---- 3. the entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_a_nan_vector_fails_its_query_alone_with_the_query_named(name):
    index, orc, stored = world(name)
    Q = MC.near_far_queries(stored, T3, 16, 11)
    Q[3, 2, 1] = np.nan
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ids, scores = np.full((16, TOPN), 7, dtype=np.uint32), np.full((16, TOPN), 3.5, dtype=np.float32)
    counts, unique, stats = np.full(16, 9, dtype=np.uint32), np.full(16, 9, dtype=np.uint32), np.zeros((16, 4), dtype=np.int32)
    L = _lib.lib()
    rc = L.hnsw_search_batch_multi(index._h, Q.ctypes.data_as(f32p), 16, T3, None, 0, TOPN, POOL, EF, ids.ctypes.data_as(u32p),
                                   scores.ctypes.data_as(f32p), counts.ctypes.data_as(u32p), unique.ctypes.data_as(u32p),
                                   C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)))
    assert rc == _lib.ERR_NAN_INPUT and L.hnsw_last_error().startswith(b"query 3:")
    assert counts[3] == 0 and unique[3] == 0 and (ids[3] == MAX).all() and np.isposinf(scores[3]).all()
    assert stats[3, 3] == _lib.ERR_NAN_INPUT
    good = np.delete(np.arange(16), 3)  # every other row is filled in
    want = index.search_batch_multi(Q[good], TOPN, POOL, EF)
    assert np.array_equal(ids[good], want[0]) and np.array_equal(scores[good].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(counts[good], want[2]) and np.array_equal(unique[good], want[3]) and (stats[good, 3] == 0).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_a_call_is_one_search_and_one_fusion(name):
    index, orc, stored = world(name)
    Q = MC.near_far_queries(stored, T3, NQ, QUERY_SEED)
    index.search_batch_multi(Q, TOPN, POOL, EF)  # (the snapshot is in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q.reshape(NQ * T3, -1), POOL, EF)
    keys = ("multi_calls", "multi_fuse_launches", "uploads")
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_multi(Q, TOPN, POOL, EF, mode="min")
    fk = kernel_of(index)
    assert log.get(fk) == 1 and fk not in plain, (dict(log), dict(plain))
    assert {k: v for k, v in log.items() if k != fk} == dict(plain), (dict(log), dict(plain))  # one search, as the plain call
    assert {k: index.stat(k) for k in keys} == {"multi_calls": before["multi_calls"] + 1,
                                                "multi_fuse_launches": before["multi_fuse_launches"] + 1,
                                                "uploads": before["uploads"]}


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_under_deletions(name):
    index, orc, stored = world(name)
    Q = MC.near_far_queries(stored, T3, 32, 13)
    found = np.asarray(orc.search_batch(Q.reshape(32 * T3, -1), 8, EF)[0])
    deleted = np.unique(found[:, 1::3].reshape(-1))
    index.mark_deleted(deleted)
    try:
        pool = 64  # the limit while ids are deleted; T * pool = 192
        c = index.search_batch(Q.reshape(32 * T3, -1), pool, 64)
        want = H.fuse_lists(Q, None, "sum", c[0].reshape(32, T3, pool), c[2].reshape(32, T3), c[3][:, 3].reshape(32, T3),
                            orc.distance_batch, TOPN, N)
        got = index.search_batch_multi(Q, TOPN, pool, 64)
        MC.assert_fused_equal(got[:4], want, name)
        assert np.array_equal(got[4], summed_stats(c[3].reshape(32, T3, 4), want[4])), "stats are the candidate call's, summed"
        assert (got[2] == TOPN).all() and not np.isin(got[0], deleted).any()
        with pytest.raises(H.HnswError) as e:
            index.search_batch_multi(Q, TOPN, pool + 1, 64)
        assert e.value.code == _lib.ERR_ARG and "pool <= 64 while ids are deleted" in str(e.value)
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_multi(Q, TOPN, 85, 128)  # nothing deleted: the unfiltered limits again
    assert (got[2] == TOPN).all()


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_cosine_option(kind):
    n, d = 1200, 24
    vs = (rand_vectors(n, d, 91) - np.float32(0.3)).astype(np.float32)
    lv = O.draw_levels(n, M, 9)
    index = H.HNSW.new(M, 32, d, kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=lv)
    # the oracle: a plain index over rows normalised beforehand by the option's arithmetic, asked with unit queries
    orc = oracle_from_product(index, SC.unit(vs), lv)
    Q = MC.near_far_queries(vs, T3, NQ, 17)
    Qu = SC.unit(Q.reshape(NQ * T3, d)).reshape(NQ, T3, d)
    c_ids, _, c_counts, c_stats = oracle_lists(orc, Qu, POOL, EF)
    w = np.tile(np.array([1.0, 0.5, 2.0], dtype=np.float32), (NQ, 1))
    for mode in ("sum", "min"):
        want = H.fuse_lists(Qu, w, mode, c_ids, c_counts, None, orc.distance_batch, TOPN, n)
        got = index.search_batch_multi(Q, TOPN, POOL, EF, weights=w, mode=mode)
        MC.assert_fused_equal(got[:4], want, "cosine " + mode)
        assert np.array_equal(got[4], summed_stats(c_stats, want[4]))
    # the primitive makes its own unit copy of the caller's raw vectors
    got, log = fuse_on_device(index, Q, w, H.FUSE_SUM, c_ids, c_counts, c_stats, TOPN)
    MC.assert_fused_equal(got[:4], H.fuse_lists(Qu, w, "sum", c_ids, c_counts, None, orc.distance_batch, TOPN, n), "cosine primitive")
    assert log.get(kernel_of(index)) == 1


def test_a_replica_handle_serves():
    import torch
    index, orc, stored = world("quant8-100")
    index.upload()
    L = _lib.lib()
    desc, there = _lib.SnapshotDesc(), _lib.SnapshotDesc()
    _lib.check(L.hnsw_snapshot_describe(index._h, C.byref(desc)))
    rep = H.HNSW.new(M, 32, index.dim, index.vec_kind)
    for i in range(7):
        there.bytes[i] = desc.bytes[i]
    for i in range(32):
        there.header[i] = desc.header[i]
    _lib.check(L.hnsw_snapshot_adopt(rep._h, C.byref(there)))

    class Mem:
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    for i in range(7):
        if desc.bytes[i]:
            a = torch.as_tensor(Mem(int(desc.ptr[i]), int(desc.bytes[i])), device="cuda:0")
            b = torch.as_tensor(Mem(int(there.ptr[i]), int(there.bytes[i])), device="cuda:0")
            b.copy_(a)
    torch.cuda.synchronize()
    _lib.check(L.hnsw_snapshot_commit(rep._h))
    T, pool = TOTALS[65]
    Q, w, ids, counts, stats = host_made_lists(stored, T, pool, 5)
    statuses = stats[:, :, 3].astype(np.uint32).view(np.int32).astype(np.int64)
    got, log = fuse_on_device(rep, Q, w, H.FUSE_SUM, ids, counts, stats, 10)
    want = H.fuse_lists(Q, w, "sum", ids, counts, statuses, orc.distance_batch, 10, N)
    MC.assert_fused_equal(got[:4], want, "replica")
    assert dict(log) == {kernel_of(index): 1}
    Qs = MC.near_far_queries(stored, T3, NQ, QUERY_SEED)
    a, b = rep.search_batch_multi(Qs, TOPN, POOL, EF), index.search_batch_multi(Qs, TOPN, POOL, EF)
    assert all(np.array_equal(x, y) for x, y in zip(a[:1] + a[2:], b[:1] + b[2:]))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- 4. capture and replay ------------------------------------------------------------------------------------------------
CAP_T, CAP_POOL = 3, 16


def cap_lists(stored, seed):
    """every query legal and every weight finite (the replayed bytes are compared, statuses included)"""
    Q, w, ids, counts, stats = host_made_lists(stored, CAP_T, CAP_POOL, seed)
    ids[4, CAP_T - 1, 0] = 7
    Q[5] = Q[4]
    stats[6, CAP_T - 1, 3] = 0
    return Q, w, ids, counts, stats


@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_the_primitive_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name):
    import torch
    index, orc, stored = world(name)
    index.upload()
    lists = {"real": cap_lists(stored, 31), "decoy": cap_lists(stored, 32)}
    names = ("Q", "w", "ids_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}
    shapes = {"ids": (NQ, TOPN), "scores": (NQ, TOPN), "counts": (NQ,), "unique": (NQ,), "stats": (NQ, 4)}

    def enqueue(i, o, stream):
        index.fuse_lists_device(NQ, CAP_T, CAP_POOL, TOPN, "sum", i["Q"], i["w"], i["ids_in"], i["counts_in"], i["stats_in"],
                                o["ids"], o["scores"], o["counts"], o["unique"], o["stats"], stream)

    def want(which):
        Q, w, ids, counts, stats = lists[which]
        f = H.fuse_lists(Q, w, "sum", ids, counts, None, orc.distance_batch, TOPN, N)
        assert (f[4] == 0).all()
        return f[0], f[1].view(np.uint32), f[2], f[3], summed_stats(stats, f[4]).astype(np.uint32)

    call = SC.Call(torch, "fuse", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {kernel_of(index): 1})


@pytest.mark.parametrize("name", ["f32-100", "quant8-100"])
def test_the_chain_search_fuse_is_two_nodes_and_replays_the_direct_calls_bytes(name):
    """inside the capture conditions of hnsw_search_batch_device (ef <= 256, nothing deleted, cosine off); both launches
    are enqueued on ONE stream, so the captured graph is one chain without parallel branches.  _finish synchronises and is
    no part of a captured graph: the direct chain is run with it as well, to the same bytes."""
    import torch
    index, orc, stored = world(name)
    index.upload()
    qs = {"real": MC.near_far_queries(stored, T3, NQ, 41), "decoy": MC.near_far_queries(stored, T3, NQ, 42)}
    inputs = {"Q": (qs["real"], qs["decoy"])}
    shapes = {"ids": (NQ, TOPN), "scores": (NQ, TOPN), "counts": (NQ,), "unique": (NQ,), "stats": (NQ, 4)}
    dev = torch.device("cuda:0")
    rows = NQ * T3
    mid = {"ids": torch.zeros((rows, POOL), dtype=torch.int32, device=dev),
           "dists": torch.zeros((rows, POOL), dtype=torch.int32, device=dev),
           "counts": torch.zeros(rows, dtype=torch.int32, device=dev),
           "stats": torch.zeros((rows, 4), dtype=torch.int32, device=dev)}

    def search_args(i, stream):
        return (i["Q"].data_ptr(), rows, POOL, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(), mid["counts"].data_ptr(),
                mid["stats"].data_ptr(), stream)

    def enqueue(i, o, stream, finish=False):
        index.search_batch_device(*search_args(i, stream))
        if finish:
            index.search_batch_device_finish(*search_args(i, stream))
        index.fuse_lists_device(NQ, T3, POOL, TOPN, "sum", i["Q"], None, mid["ids"], mid["counts"], mid["stats"], o["ids"],
                                o["scores"], o["counts"], o["unique"], o["stats"], stream)

    def want(which):
        c_ids, _, c_counts, c_stats = oracle_lists(orc, qs[which], POOL, EF)
        f = H.fuse_lists(qs[which], None, "sum", c_ids, c_counts, None, orc.distance_batch, TOPN, N)
        return f[0], f[1].view(np.uint32), f[2], f[3], summed_stats(c_stats, f[4]).astype(np.uint32)

    call = SC.Call(torch, "chain", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    # the direct chain with _finish in it
    call.load("real")
    call.poison()
    enqueue(call.inp, call.out, torch.cuda.current_stream().cuda_stream, finish=True)
    torch.cuda.synchronize()
    assert SC.verdict(call.arrays(copies=False), want("real")) is None
    with H.kernel_log() as plain:
        index.search_batch_device(*search_args(call.inp, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert sum(plain.values()) == 1, dict(plain)
    expected = dict(plain)
    expected[kernel_of(index)] = 1
    capture_and_replay(torch, call, want, expected)
