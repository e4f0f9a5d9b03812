"""Search from stored rows on the GPU (include/hnsw_mi355x.h, "search from stored rows"), held to the numpy restatements
of the fold and the drop (hnsw_rs_amd.from_rows; tests/test_from_rows_host.py holds those to plain loops) over the CPU
oracle's rows (OracleHNSW.get_vals) and search (OracleHNSW.search_batch).  All comparisons are exact: ids, distance
BITS, counts, counters and statuses; of a NaN element only that it is one (the contract does not fix a NaN's bits).
  1. hnsw_compose_rows_device alone: one launch and nothing else, guard words, a bad id fails its query alone;
  2. hnsw_drop_ids_device alone over the host test's sweep;
  3. search_batch_by_id and two-term searches against the drop of the ORACLE's lists;
  4. the entry point: exclude = 0, launch accounting, deletions, the cosine option, a replica handle, knn_graph;
  5. capture and replay of each primitive and of the chain compose -> search -> drop on a torch stream."""
import ctypes as C
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import from_rows_cases as FC
from tests import stream_cases as SC
from tests.util import assert_search_equal, oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A  # (as a float 1.5e16, as an id beyond every index here)
GUARD = 64  # words behind every output that no launch may write
N, M = 1500, 16
SHAPES = {"f32-16": (H.VEC_F32, 16), "f32-100": (H.VEC_F32, 100), "quant8-40": (H.VEC_QUANT8, 40),
          "quant8-100": (H.VEC_QUANT8, 100)}
TOPN, EF = 10, 32
MERGE_KERNEL = "hx_filt_merge_kernel"


def kernel_of(index):
    return "hx_distance_kernel<%d>" % index.vec_kind


@functools.lru_cache(maxsize=None)
def world(name):
    """an index of 1500 points whose rows 1400 .. 1499 repeat rows 0 .. 99, the oracle holding its graph, and the rows as
    the oracle returns them.  Built once, shared, left unchanged (a test that deletes ids puts them back)."""
    kind, d = SHAPES[name]
    vs = rand_vectors(N, d, 61 + d)
    vs[1400:1500] = vs[0:100]
    lv = O.draw_levels(N, M, 61)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(vs, 4, False, levels=lv)
    orc = oracle_from_product(index, vs, lv)
    stored = np.stack([orc.get_vals(i) for i in range(N)]).astype(np.float32)
    stored.setflags(write=False)
    return index, orc, stored


def up(a):  # (uint32 and float32 travel as int32: the bits are what the kernels read)
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).copy()).to(torch.device("cuda:0"))


def guarded(sizes):
    import torch
    dev = torch.device("cuda:0")
    return {k: torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev) if n else None for k, n in sizes.items()}


def unguard(out, sizes):
    got = {}
    for k, t in out.items():
        if t is None:
            got[k] = None
            continue
        a = t.cpu().numpy().view(np.uint32)
        assert (a[sizes[k]:] == SENTINEL).all(), "%s: a guard word behind the output was written" % k
        assert not (a[:sizes[k]] == SENTINEL).any(), "%s: an output word was left unwritten" % k
        got[k] = a[:sizes[k]]
    return got


def assert_rows_equal(got, want, what):
    """bit for bit, but for the bits of a NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: the NaN elements differ" % what
    g, w = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere((g != w) & ~nan)
    assert bad.size == 0, "%s: %d elements differ, first at %s: %08x vs %08x" % (
        what, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


# ---- 1. compose alone ---------------------------------------------------------------------------------------------------
def compose_on_device(index, src, weights, want_status=True):
    import torch
    nq, width = src.shape
    d_src, d_w = up(src), None if weights is None else up(weights)
    sizes = {"Q": nq * index.dim, "status": nq if want_status else 0}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.compose_rows_device(nq, width, d_src, d_w, out["Q"], out["status"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    return got["Q"].view(np.float32).reshape(nq, index.dim), None if got["status"] is None else got["status"].view(np.int32), log


@pytest.mark.parametrize("width", [1, 2, 5, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_compose_alone_is_the_restatement_bit_for_bit(name, width):
    index, orc, stored = world(name)
    index.upload()
    launches = index.stat("from_rows_compose_launches")
    src, w = FC.compose_slots(width, N, 300 + width, nq=70)  # (more queries than one block's worth of anything)
    src[12:, :] = np.random.default_rng(width).integers(0, N, (58, width))
    src[20, :] = np.arange(1400, 1400 + width)  # copied rows
    for k, weights in enumerate((w, None)):
        got_rows, got_status, log = compose_on_device(index, src, weights, want_status=k == 0)
        assert dict(log) == {kernel_of(index): 1}, dict(log)
        want_rows, want_status = H.compose_rows(src, weights, lambda i: stored[i], N)
        assert_rows_equal(got_rows, want_rows, "%s width=%d weights=%s" % (name, width, weights is not None))
        if got_status is not None:
            assert np.array_equal(got_status, want_status)
        # a bad id fails its query alone: a row of zeros, its neighbours untouched
        assert want_status[4] == want_status[5] == _lib.ERR_ARG and (want_status != 0).sum() == 2
        assert (got_rows[4].view(np.uint32) == 0).all() and (got_rows[5].view(np.uint32) == 0).all()
        if weights is not None:
            assert np.isnan(got_rows[9]).any()  # the NaN weight reaches the row
    if width == 1:  # one slot, no weights: the stored row itself
        assert np.array_equal(got_rows[6].view(np.uint32), stored[11].view(np.uint32))
    assert index.stat("from_rows_compose_launches") == launches + 2 and index.stat("from_rows_calls") == 0


# ---- 2. drop alone ------------------------------------------------------------------------------------------------------
def drop_on_device(ids, dists, counts, stats, ex, n_out, src_st, want_extra=True):
    import torch
    nq, n_in = ids.shape
    width = ex.shape[1]
    d_in = (up(ids), up(dists), None if counts is None else up(counts), None if stats is None else up(stats.astype(np.uint32)))
    sizes = {"ids": nq * n_out, "dists": nq * n_out, "counts": nq if want_extra else 0, "dropped": nq if want_extra else 0,
             "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        H.HNSW.drop_ids_device(nq, n_in, n_out, width, up(ex), None if src_st is None else up(src_st), d_in[0], d_in[1], d_in[2],
                               d_in[3], out["ids"], out["dists"], out["counts"], out["dropped"], out["stats"],
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shape = (nq, n_out)
    return (got["ids"].reshape(shape), got["dists"].view(np.float32).reshape(shape), got["counts"], got["dropped"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4).view(np.int32).astype(np.int64)), log


@pytest.mark.parametrize("n_in,width", FC.drop_sweep())
def test_drop_alone_is_the_restatement(n_in, width):
    for with_counts in (True, False):
        ids, dists, counts, statuses, ex, src_st = FC.drop_lists(n_in, width, with_counts, seed=1000 * n_in + 10 * width + with_counts)
        stats = np.random.default_rng(n_in).integers(2 ** 31, 2 ** 32, (FC.NQ, 4)).astype(np.int64)
        stats[:, 3] = statuses
        for n_out in FC.n_outs(n_in):
            for src in (None, src_st):
                what = "n_in=%d width=%d counts=%s n_out=%d src=%s" % (n_in, width, with_counts, n_out, src is not None)
                got, log = drop_on_device(ids, dists, counts, stats, ex, n_out, src)
                assert dict(log) == {MERGE_KERNEL: 1}, (what, dict(log))
                want = H.drop_ids(ids, dists, counts, statuses, ex, n_out, src)
                FC.assert_drop_equal(got, want, what)
                want_stats = stats.copy()
                want_stats[:, 3] = want[4]  # (the compose status, where it failed, is the one the record carries)
                want_stats[:, :3] &= 0xFFFFFFFF
                got[4][:, :3] &= 0xFFFFFFFF
                assert np.array_equal(got[4], want_stats), what
        # without stats and the optional outputs: the same rows (query 6 is an ordinary one here)
        n_out = FC.n_outs(n_in)[1 if n_in > 1 else 0]
        got, log = drop_on_device(ids, dists, counts, None, ex, n_out, None, want_extra=False)
        want = H.drop_ids(ids, dists, counts, None, ex, n_out)
        FC.assert_drop_equal((got[0], got[1], want[2]), want, "bare n_in=%d width=%d" % (n_in, width))
        assert got[2] is None and got[3] is None and got[4] is None and dict(log) == {MERGE_KERNEL: 1}


# ---- 3. the searches against the drop of the oracle's lists ------------------------------------------------------------
SOURCES = np.arange(0, N, 23, dtype=np.uint32)  # 66 of them; 1403, 1426, 1449, 1472 and 1495 are copies of earlier rows


@pytest.mark.parametrize("name", list(SHAPES))
def test_search_by_id_is_the_drop_of_the_oracles_lists(name):
    index, orc, stored = world(name)
    assert SOURCES.shape[0] == 66
    cand = orc.search_batch(stored[SOURCES], TOPN + 1, EF)
    c_ids = np.asarray(cand[0])
    # what keeps the comparison from passing vacuously, met by the oracle alone: every source is found in its own list,
    # and a source whose twin has the lower id is not the first entry of it
    assert all(int(s) in c_ids[q].tolist() for q, s in enumerate(SOURCES.tolist()))
    late = [q for q, s in enumerate(SOURCES.tolist()) if s >= 1400]
    assert len(late) == 5 and all(c_ids[q, 0] == SOURCES[q] - 1400 and c_ids[q, 0] != SOURCES[q] for q in late)
    w = H.drop_ids(cand[0], cand[1], cand[2], None, SOURCES.reshape(-1, 1), TOPN)
    assert (w[3] == 1).all() and (w[2] == TOPN).all()
    got = index.search_batch_by_id(SOURCES, TOPN, EF)
    assert_search_equal(got, (w[0], w[1], w[2], cand[3]), name)
    assert (got[3][:, 3] == 0).all() and not any(int(s) in got[0][q].tolist() for q, s in enumerate(SOURCES.tolist()))


def pairs_of(orc, stored):
    """64 (id, its nearest neighbour) pairs, then 64 random pairs"""
    a = np.arange(5, 5 + 64 * 17, 17, dtype=np.uint32)
    near = np.asarray(orc.search_batch(stored[a], 2, EF)[0])
    b = np.where(near[:, 0] == a, near[:, 1], near[:, 0]).astype(np.uint32)
    rng = np.random.default_rng(9)
    return np.concatenate([np.stack([a, b], axis=1), rng.integers(0, N, (64, 2)).astype(np.uint32)])


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_terms_with_equal_weights(name):
    index, orc, stored = world(name)
    src = pairs_of(orc, stored)
    weights = np.full(src.shape, 0.5, dtype=np.float32)
    rows, st = H.compose_rows(src, weights, lambda i: stored[i], N)
    assert (st == 0).all()
    cand = orc.search_batch(rows, TOPN + 2, EF)
    w = H.drop_ids(cand[0], cand[1], cand[2], None, src, TOPN)
    both = np.flatnonzero(w[3][:64] == 2)
    assert both.size >= 1, "no neighbour pair has both sources among the oracle's candidates"
    got = index.search_batch_from_rows(src, weights, TOPN, EF)
    assert_search_equal(got, (w[0], w[1], w[2], cand[3]), name)
    assert not any(np.isin(got[0][q], src[q]).any() for q in both.tolist())


# ---- 4. the entry point -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_without_exclusion_it_is_search_batch_of_the_composed_rows(name):
    index, orc, stored = world(name)
    src = pairs_of(orc, stored)[32:96]
    weights = np.tile(np.array([1.5, -0.5], dtype=np.float32), (src.shape[0], 1))
    rows, _ = H.compose_rows(src, weights, lambda i: stored[i], N)
    drops = index.stat("from_rows_drop_launches")
    with H.kernel_log() as log:
        got = index.search_batch_from_rows(src, weights, TOPN, EF, exclude=False)
    assert_search_equal(got, orc.search_batch(rows, TOPN, EF), name)
    assert_search_equal(got, index.search_batch(rows, TOPN, EF), name + " product")
    assert MERGE_KERNEL not in log and log.get(kernel_of(index)) == 1 and index.stat("from_rows_drop_launches") == drops
    got = index.search_batch_by_id(SOURCES, TOPN, EF, exclude_self=False)
    assert_search_equal(got, orc.search_batch(stored[SOURCES], TOPN, EF), name + " by id")


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_a_nan_weight_fails_its_query_alone_with_the_searchs_own_status(name):
    index, orc, stored = world(name)
    src = np.ascontiguousarray(pairs_of(orc, stored)[:16])
    w = np.full(src.shape, 0.5, dtype=np.float32)
    w[3, 1] = np.nan
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ids, dists = np.full((16, TOPN), 7, dtype=np.uint32), np.full((16, TOPN), 3.5, dtype=np.float32)
    counts, stats = np.full(16, 9, dtype=np.uint32), np.zeros((16, 4), dtype=np.int32)
    L = _lib.lib()
    rc = L.hnsw_search_batch_from_rows(index._h, src.ctypes.data_as(u32p), w.ctypes.data_as(f32p), 16, 2, TOPN, EF, 1,
                                       ids.ctypes.data_as(u32p), dists.ctypes.data_as(f32p), counts.ctypes.data_as(u32p),
                                       C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)))
    assert rc == _lib.ERR_NAN_INPUT and L.hnsw_last_error().startswith(b"query 3:")
    assert counts[3] == 0 and (ids[3] == MAX).all() and np.isposinf(dists[3]).all() and stats[3, 3] == _lib.ERR_NAN_INPUT
    good = np.delete(np.arange(16), 3)  # every other row is filled in
    want = index.search_batch_from_rows(src[good], w[good], TOPN, EF)
    assert np.array_equal(ids[good], want[0]) and np.array_equal(dists[good].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(counts[good], want[2]) and (stats[good, 3] == 0).all() and (counts[good] == TOPN).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_a_call_is_one_compose_the_search_and_one_drop(name):
    index, orc, stored = world(name)
    index.search_batch_by_id(SOURCES, TOPN, EF)  # (the snapshot is in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(stored[SOURCES], TOPN + 1, EF)
    keys = ("from_rows_calls", "from_rows_compose_launches", "from_rows_drop_launches", "uploads")
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_by_id(SOURCES, TOPN, EF)
    ck = kernel_of(index)
    assert log.get(ck) == 1 and log.get(MERGE_KERNEL) == 1, dict(log)
    assert ck not in plain and MERGE_KERNEL not in plain
    assert {k: v for k, v in log.items() if k not in (ck, MERGE_KERNEL)} == dict(plain), (dict(log), dict(plain))
    after = {k: index.stat(k) for k in keys}
    assert after == {"from_rows_calls": before["from_rows_calls"] + 1,
                     "from_rows_compose_launches": before["from_rows_compose_launches"] + 1,
                     "from_rows_drop_launches": before["from_rows_drop_launches"] + 1, "uploads": before["uploads"]}


@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_under_deletions(name):
    index, orc, stored = world(name)
    src = SOURCES[:32]
    found = np.asarray(orc.search_batch(stored[src], 8, EF)[0])
    deleted = np.unique(np.concatenate([found[:, 1::3].reshape(-1), src[5:9]]))  # neighbours, and four of the sources
    index.mark_deleted(deleted)
    try:
        n = 63  # n + width = 64: the limit while ids are deleted
        c = index.search_batch(stored[src], n + 1, 64)
        w = H.drop_ids(c[0], c[1], c[2], c[3][:, 3], src.reshape(-1, 1), n)
        got = index.search_batch_by_id(src, n, 64)
        FC.assert_drop_equal(got[:3], w, name)
        assert np.array_equal(got[3], c[3]), "stats are the candidate call's"
        assert not np.isin(got[0][got[0] != MAX], deleted).any()
        # a deleted source is a legal one: no search returns it, nothing is dropped, the list is cut to n
        gone = np.isin(src, deleted)
        assert gone[5:9].all() and not gone.all()
        for q in np.flatnonzero(gone).tolist():
            assert w[3][q] == 0 and np.array_equal(got[0][q], c[0][q, :n])
        assert (w[3][~gone] == 1).all()
        with pytest.raises(H.HnswError) as e:
            index.search_batch_by_id(src, n + 1, 64)
        assert e.value.code == _lib.ERR_ARG and "while ids are deleted" in str(e.value)
        two = np.stack([src, src[::-1]], axis=1)
        got = index.search_batch_from_rows(two, None, 62, 64)
        rows, _ = H.compose_rows(two, None, lambda i: stored[i], N)
        c = index.search_batch(rows, 64, 64)
        FC.assert_drop_equal(got[:3], H.drop_ids(c[0], c[1], c[2], c[3][:, 3], two, 62), name + " two terms")
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_by_id(src, 64, 128)  # nothing deleted: the unfiltered limits again
    assert (got[2] == 64).all()


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_cosine_option(kind):
    n, d = 1200, 24
    vs = (rand_vectors(n, d, 91) - np.float32(0.3)).astype(np.float32)
    lv = O.draw_levels(n, M, 9)
    index = H.HNSW.new(M, 32, d, kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=lv)
    # the oracle over rows normalised beforehand by the option's arithmetic (it quantises the unit rows itself)
    orc = oracle_from_product(index, SC.unit(vs), lv)
    src = np.stack([np.arange(0, 640, 10), np.arange(3, 643, 10)], axis=1).astype(np.uint32)
    weights = np.tile(np.array([1.0, 0.25], dtype=np.float32), (src.shape[0], 1))
    rows, _ = H.compose_rows(src, weights, orc.get_vals, n)
    assert np.array_equal(orc.get_vals(7).view(np.uint32), index.get_point(7).get_vals().view(np.uint32))  # the stored unit row
    cand = orc.search_batch(SC.unit(rows), TOPN + 2, EF)
    w = H.drop_ids(cand[0], cand[1], cand[2], None, src, TOPN)
    assert (w[3] >= 1).all()
    got = index.search_batch_from_rows(src, weights, TOPN, EF)
    assert_search_equal(got, (w[0], w[1], w[2], cand[3]), "cosine")


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
    got, want = rep.search_batch_by_id(SOURCES, TOPN, EF), index.search_batch_by_id(SOURCES, TOPN, EF)
    assert_search_equal(got, want, "replica")
    src, w = FC.compose_slots(5, N, 77, nq=16)
    rows, status, _ = compose_on_device(rep, src, w)
    want_rows, want_status = H.compose_rows(src, w, lambda i: stored[i], N)
    assert_rows_equal(rows, want_rows, "replica compose")
    assert np.array_equal(status, want_status)
    with pytest.raises(H.HnswError) as e:
        rep.search_batch_by_id([N], TOPN, EF)
    assert e.value.code == _lib.ERR_ARG and "1500 points" in str(e.value)


def test_knn_graph_in_chunks_is_one_call_over_all_ids():
    index, orc, stored = world("f32-16")
    calls = index.stat("from_rows_calls")
    whole = index.search_batch_by_id(np.arange(N, dtype=np.uint32), TOPN, EF)
    got = index.knn_graph(TOPN, EF, chunk=512)  # 512, 512 and a ragged 476
    assert index.stat("from_rows_calls") == calls + 4
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1].view(np.uint32), whole[1].view(np.uint32))
    assert np.array_equal(got[2], whole[2]) and got[0].shape == (N, TOPN)
    assert not (got[0] == np.arange(N)[:, None]).any()  # no row names itself
    some = index.knn_graph(TOPN, EF, chunk=7, ids=SOURCES[:20], exclude_self=False)
    assert np.array_equal(some[0], index.search_batch_by_id(SOURCES[:20], TOPN, EF, False)[0])
    assert (some[0][:5, 0] == SOURCES[:5]).all()  # (f32: a row is at distance 0 from itself, the lower id first)


# ---- 5. capture and replay ----------------------------------------------------------------------------------------------
CAP_WIDTH = 3


def capture_and_replay(torch, call, want, direct_kernels):
    """the direct call on the current stream against `want`, then captured on a side stream as exactly the launches of
    direct_kernels, then replayed over real, decoy and real inputs: the bytes of the direct calls"""
    direct = {}
    for which in ("real", "decoy"):
        call.load(which)
        call.poison()
        call.enqueue(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        direct[which] = call.arrays(copies=False)
        assert SC.verdict(direct[which], want(which)) is None, which
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call.load("decoy")
        s.synchronize()
    with H.kernel_log() as log:
        with torch.cuda.graph(g, stream=s):
            call.enqueue(torch.cuda.current_stream().cuda_stream)
    assert dict(log) == direct_kernels, "the captured launches: %s" % dict(log)
    with torch.cuda.stream(s):
        for which in ("real", "decoy", "real"):
            call.load(which)
            call.poison()
            g.replay()
            s.synchronize()
            got = call.arrays(copies=False)
            assert all(np.array_equal(a, b) for a, b in zip(got, direct[which])), "replay over %s" % which


def cap_slots(seed):
    src, w = FC.compose_slots(CAP_WIDTH, N, seed, nq=SC.NQ)
    w[8], w[9] = np.float32(0.5), np.float32(-1.25)  # (finite weights: a NaN's bits are no part of the comparison)
    return src, w


@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_compose_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name):
    import torch
    index, orc, stored = world(name)
    index.upload()
    slots = {"real": cap_slots(31), "decoy": cap_slots(32)}
    inputs = {"src": (slots["real"][0], slots["decoy"][0]), "w": (slots["real"][1], slots["decoy"][1])}
    shapes = {"Q": (SC.NQ, index.dim), "status": (SC.NQ,)}

    def enqueue(i, o, stream):
        index.compose_rows_device(SC.NQ, CAP_WIDTH, i["src"], i["w"], o["Q"], o["status"], stream)

    def want(which):
        rows, st = H.compose_rows(slots[which][0], slots[which][1], lambda i: stored[i], N)
        return rows.view(np.uint32), st.astype(np.uint32)

    call = SC.Call(torch, "compose", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {kernel_of(index): 1})


def test_drop_is_captured_as_one_launch_and_replays_the_direct_calls_bytes():
    import torch
    lists = {"real": SC.pool_lists(31, N), "decoy": SC.pool_lists(32, N)}
    ex = {k: np.stack([v[0][:, 0], v[0][:, 7], np.full(SC.NQ, MAX, dtype=np.uint32)], axis=1) for k, v in lists.items()}
    names = ("ids_in", "dists_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}
    inputs["ex"] = (ex["real"], ex["decoy"])
    shapes = {"ids": (SC.NQ, TOPN), "dists": (SC.NQ, TOPN), "counts": (SC.NQ,), "dropped": (SC.NQ,), "stats": (SC.NQ, 4)}

    def enqueue(i, o, stream):
        H.HNSW.drop_ids_device(SC.NQ, SC.POOL, TOPN, 3, i["ex"], None, i["ids_in"], i["dists_in"], i["counts_in"], i["stats_in"],
                               o["ids"], o["dists"], o["counts"], o["dropped"], o["stats"], stream)

    def want(which):
        ids, dists, counts, stats = lists[which]
        w = H.drop_ids(ids, dists, counts, None, ex[which], TOPN)
        return w[0], w[1].view(np.uint32), w[2], w[3], stats.astype(np.uint32)

    call = SC.Call(torch, "drop", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {MERGE_KERNEL: 1})


@pytest.mark.parametrize("name", ["f32-100", "quant8-100"])
def test_the_chain_compose_search_drop_is_three_nodes_and_replays_the_direct_calls_bytes(name):
    """inside the header's capture conditions (ef <= 256, nothing deleted, cosine off); the three launches are enqueued on
    ONE stream, so the captured graph is one chain without parallel branches"""
    import torch
    index, orc, stored = world(name)
    index.upload()
    slots = {"real": cap_slots(41), "decoy": cap_slots(42)}
    for s in slots.values():  # every query legal: the chain's search gets composed rows only
        s[0][4, :], s[0][5, :] = np.array([7, MAX, 1409]), np.array([1, 2, 3])
    inputs = {"src": (slots["real"][0], slots["decoy"][0]), "w": (slots["real"][1], slots["decoy"][1])}
    n_cand = TOPN + CAP_WIDTH
    shapes = {"ids": (SC.NQ, TOPN), "dists": (SC.NQ, TOPN), "counts": (SC.NQ,), "dropped": (SC.NQ,), "stats": (SC.NQ, 4)}
    dev = torch.device("cuda:0")
    mid = {"Q": torch.zeros((SC.NQ, index.dim), dtype=torch.float32, device=dev),
           "status": torch.zeros(SC.NQ, dtype=torch.int32, device=dev),
           "ids": torch.zeros((SC.NQ, n_cand), dtype=torch.int32, device=dev),
           "dists": torch.zeros((SC.NQ, n_cand), dtype=torch.int32, device=dev),
           "counts": torch.zeros(SC.NQ, dtype=torch.int32, device=dev),
           "stats": torch.zeros((SC.NQ, 4), dtype=torch.int32, device=dev)}

    def enqueue(i, o, stream):
        index.compose_rows_device(SC.NQ, CAP_WIDTH, i["src"], i["w"], mid["Q"], mid["status"], stream)
        index.search_batch_device(mid["Q"].data_ptr(), SC.NQ, n_cand, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(),
                                  mid["counts"].data_ptr(), mid["stats"].data_ptr(), stream)
        H.HNSW.drop_ids_device(SC.NQ, n_cand, TOPN, CAP_WIDTH, i["src"], mid["status"], mid["ids"], mid["dists"], mid["counts"],
                               mid["stats"], o["ids"], o["dists"], o["counts"], o["dropped"], o["stats"], stream)

    def want(which):
        src, w = slots[which]
        rows, st = H.compose_rows(src, w, lambda i: stored[i], N)
        assert (st == 0).all()
        cand = orc.search_batch(rows, n_cand, EF)
        d = H.drop_ids(cand[0], cand[1], cand[2], None, src, TOPN, st)
        stats = np.concatenate([np.asarray(cand[3])[:, :3].astype(np.uint32), np.zeros((SC.NQ, 1), dtype=np.uint32)], axis=1)
        return d[0], d[1].view(np.uint32), d[2], d[3], stats

    call = SC.Call(torch, "chain", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    assert (want("real")[3] >= 1).any() and (want("decoy")[3] >= 1).any()
    with H.kernel_log() as plain:
        index.search_batch_device(mid["Q"].data_ptr(), SC.NQ, n_cand, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(),
                                  mid["counts"].data_ptr(), mid["stats"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert sum(plain.values()) == 1, dict(plain)
    expected = dict(plain)
    expected[kernel_of(index)] = 1
    expected[MERGE_KERNEL] = 1
    capture_and_replay(torch, call, want, expected)
