"""Partitioned search on the GPU (include/hnsw_mi355x.h, "partitioned search"), held to the numpy restatement of the
merge (tests/partitioned_restate.py):
  1. hnsw_merge_topk_device alone, bit for bit, over synthetic lists built to hold every edge the merge has, and the
     kernel log: one launch of hx_filt_merge_kernel and nothing else;
  2. PartitionedIndex.search_batch (hnsw_search_batch_shards) end to end against the CPU oracle's search per shard;
  3. exactness across shards: the shards' brute-force lists merged are the unsplit index's brute force;
  4. deletions routed to the shards;
  5. PartitionedSearcher over a one-rank nccl (= RCCL) communicator with the HIP search and the HIP merge."""
import functools
import os
import socket
import sys

import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests.partitioned_restate import merge_restate
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
NQ = 37
FLT_MAX_BITS = 0x7F7FFFFF


# ---- 1. the merge alone ----------------------------------------------------------------------------------------------
def synthetic_lists(S, n, with_counts, seed):
    """[S][NQ][n] lists as S shards could return them, with the merge's edges planted:
    query 3: shard 0 has count 0;  query 5: every shard has count 0;  query 7: shard 1 repeats shard 0's list (the same
    keys from two shards, when the id map lets them overlap);  query 9: the last shard's status blanks it;  query 11:
    shards 0 and 1 both failed (the lower one's status wins);  query 13: a count above n (clamped);  distances from a
    handful of values, 0.0 and FLT_MAX among them, so that equal distance bits across shards are the rule and the id
    decides;  counters near 2^32 so that the sums wrap.  With counts, the entries beyond a count hold live-looking
    ids that must not be read as present; without, they are the pad."""
    rng = np.random.default_rng(seed)
    values = np.array([0.0, 0.25, 0.5, 1.0, 3.0, 0.0], dtype=np.float32)
    values[5] = np.array([FLT_MAX_BITS], dtype=np.uint32).view(np.float32)[0]
    ids = np.zeros((S, NQ, n), dtype=np.uint32)
    dists = np.zeros((S, NQ, n), dtype=np.float32)
    counts = np.zeros((S, NQ), dtype=np.uint32)
    for s in range(S):
        for q in range(NQ):
            c = int(rng.integers(0, n + 1))
            if q == 5 or (q == 3 and s == 0):
                c = 0
            loc = rng.choice(5 * n, n, replace=False).astype(np.uint32)  # distinct local ids, as a search returns
            d = values[rng.integers(0, len(values), n)]
            order = np.lexsort((loc[:c], d[:c].view(np.uint32)))  # the present part sorted by (bits, id)
            loc[:c], d[:c] = loc[:c][order], d[:c][order]
            if not with_counts:
                loc[c:], d[c:] = MAX, np.inf
            ids[s, q], dists[s, q], counts[s, q] = loc, d, c
    if S > 1:
        ids[1, 7], dists[1, 7], counts[1, 7] = ids[0, 7], dists[0, 7], counts[0, 7]
    if with_counts:
        counts[S - 1, 13] = n + 5
    stats = rng.integers(2 ** 31, 2 ** 32, (S, NQ, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    stats[S - 1, 9, 3] = -2
    if S > 1:
        stats[0, 11, 3], stats[1, 11, 3] = -11, -3
    return ids, dists, counts, stats


def id_map(S, which):
    """'strided': the round-robin map, but with shards 0 and 1 on the same ids (overlapping shards); 'high': blocks from
    0xF0000000, ids above 2^31, shards 0 and 1 overlapping as well"""
    if which == "strided":
        base, stride = np.arange(S, dtype=np.uint32), np.full(S, S, dtype=np.uint32)
    else:
        base, stride = (0xF0000000 + 0x100000 * np.arange(S)).astype(np.uint32), None
    if S > 1:
        base[1] = base[0]
    return base, stride


@pytest.mark.parametrize("n", [1, 10, 63, 64])
@pytest.mark.parametrize("S", [1, 2, 3, 8, 64])
def test_merge_alone_is_the_restatement_bit_for_bit(S, n):
    import torch
    dev = torch.device("cuda:0")

    def up(a):  # (uint32 travels as int32: the bits are what the kernel reads)
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.dtype == np.float32 else a.view(np.int32)).to(dev)

    for with_counts in (True, False):
        ids, dists, counts, stats = synthetic_lists(S, n, with_counts, seed=1000 * S + n)
        d_in = up(ids), up(dists), up(counts), up(stats.astype(np.uint32))
        for which in ("strided", "high"):
            base, stride = id_map(S, which)
            want = merge_restate(ids, dists, counts if with_counts else None, stats, base, stride, n)
            o_ids = torch.full((NQ, n), 7, dtype=torch.int32, device=dev)
            o_dists = torch.full((NQ, n), 3.5, dtype=torch.float32, device=dev)
            o_counts = torch.full((NQ,), 9, dtype=torch.int32, device=dev)
            o_stats = torch.full((NQ, 4), 5, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            with H.kernel_log() as log:
                H.merge_topk(S, NQ, n, d_in[0], d_in[1], d_in[2] if with_counts else None, d_in[3], base, stride, o_ids,
                             o_dists, o_counts, o_stats, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
            what = "S=%d n=%d counts=%s map=%s" % (S, n, with_counts, which)
            assert dict(log) == {"hx_filt_merge_kernel": 1}, (what, dict(log))
            g_ids, g_bits = o_ids.cpu().numpy().view(np.uint32), o_dists.cpu().numpy().view(np.uint32)
            g_counts, g_stats = o_counts.cpu().numpy().view(np.uint32), o_stats.cpu().numpy().astype(np.int64)
            g_stats[:, :3] &= 0xFFFFFFFF
            assert np.array_equal(g_counts, want[2]), what
            assert np.array_equal(g_ids, want[0]), what
            assert np.array_equal(g_bits, want[1].view(np.uint32)), what
            assert np.array_equal(g_stats, want[3]), what
            # the planted edges did what they are there for
            assert g_counts[5] == 0 and g_counts[9] == 0 and g_stats[9, 3] == -2
            assert (g_ids[9] == MAX).all() and np.isposinf(o_dists.cpu().numpy()[9]).all()
            keys = ((g_bits.astype(np.uint64) << np.uint64(32)) | g_ids).astype(np.int64)  # (bits of a distance: below 2^31)
            for q in range(NQ):  # every distinct key once, ascending
                assert (np.diff(keys[q, :g_counts[q]]) > 0).all(), (what, q)
            if S > 1:
                assert g_stats[11, 3] == -11
            if S == 2:  # shard 1 repeated shard 0's list on the same ids: each key once
                assert g_counts[7] == min(int(counts[0, 7]), n), what
            if which == "high":
                assert (g_ids[g_ids != MAX] >= 0xF0000000).all()
    # without stats, and without the optional count output: the same rows, nothing else written
    base, stride = id_map(S, "strided")
    want = merge_restate(ids, dists, None, None, base, stride, n)
    o_ids = torch.full((NQ, n), 7, dtype=torch.int32, device=dev)
    o_dists = torch.full((NQ, n), 3.5, dtype=torch.float32, device=dev)
    with H.kernel_log() as log:
        H.merge_topk(S, NQ, n, d_in[0], d_in[1], None, None, base, stride, o_ids, o_dists)
        torch.cuda.synchronize()
    assert dict(log) == {"hx_filt_merge_kernel": 1}
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(o_dists.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


# ---- 2 - 4: PartitionedIndex against the oracle ---------------------------------------------------------------------
D, M, K, EF, NQ_E2E = 20, 8, 10, 32, 64
LAYOUTS = {"contiguous": (3000, 3), "strided": (3001, 4)}


@functools.lru_cache(maxsize=None)
def world(kind, layout):
    """the partitioned index of a layout, its rows and queries, and what the oracle says: every shard's graph searched by
    the CPU oracle, the lists merged by the restatement (computed once, shared, left unchanged)"""
    N, S = LAYOUTS[layout]
    vs, lv, Q = rand_vectors(N, D, 21), O.draw_levels(N, M, 21), rand_vectors(NQ_E2E, D, 22)
    p = H.PartitionedIndex.build(vs, S, M, 32, kind, layout=layout, levels=lv, nb_threads=4)
    per = []
    for k, sh in enumerate(p.shards):
        rows = np.arange(N)[p.to_local(np.arange(N))[0] == k]
        assert np.array_equal(p.to_global(k, np.arange(rows.size)), rows)
        orc = oracle_from_product(sh, vs[rows], lv[rows])
        ids, dists, counts, st = orc.search_batch(Q, K, EF)
        per.append((ids, dists, counts, np.concatenate([st.astype(np.int64), np.zeros((NQ_E2E, 1), dtype=np.int64)], axis=1)))
    want = merge_restate(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), np.stack([x[2] for x in per]),
                         np.stack([x[3] for x in per]), p.id_base, p.id_stride, K)
    for a in want:
        a.setflags(write=False)
    return p, vs, lv, Q, want


def assert_rows_equal(got, want, what):
    assert np.array_equal(got[2], want[2]), what + ": counts"
    assert np.array_equal(got[0], want[0]), what + ": ids"
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), want[1].view(np.uint32)), what + ": distance bits"
    assert np.array_equal(np.asarray(got[3]).astype(np.int64), want[3]), what + ": counters and status"


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_search_batch_is_the_oracle_per_shard_merged(kind, layout):
    p, vs, lv, Q, want = world(kind, layout)
    calls, merges = p.shards[0].stat("shard_calls"), p.shards[0].stat("shard_merges")
    with H.kernel_log() as log:
        got = p.search_batch(Q, K, EF)
    assert log.get("hx_filt_merge_kernel") == 1, dict(log)
    assert_rows_equal(got, want, "kind %d %s" % (kind, layout))
    assert (want[2] == K).all() and len(set((p.to_local(want[0].reshape(-1))[0]).tolist())) == len(p.shards)
    assert p.shards[0].stat("shard_calls") == calls + 1 and p.shards[0].stat("shard_merges") == merges + 1
    assert p.shards[1].stat("shard_calls") == 0


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_brute_force_lists_merged_are_the_unsplit_brute_force(kind):
    import torch
    dev = torch.device("cuda:0")
    p, vs, lv, Q, _ = world(kind, "strided")
    N, S = LAYOUTS["strided"]
    whole = H.HNSW.new(M, 32, D, kind).insert_bulk(vs, 4, False, levels=lv)
    w_ids, w_d = whole.brute_force(Q, K)
    lists = [sh.brute_force(Q, K) for sh in p.shards]
    d_ids = torch.from_numpy(np.stack([x[0] for x in lists]).view(np.int32)).to(dev)
    d_d = torch.from_numpy(np.stack([x[1] for x in lists])).to(dev)
    o_ids = torch.empty((NQ_E2E, K), dtype=torch.int32, device=dev)
    o_d = torch.empty((NQ_E2E, K), dtype=torch.float32, device=dev)
    o_c = torch.empty(NQ_E2E, dtype=torch.int32, device=dev)
    H.merge_topk(S, NQ_E2E, K, d_ids, d_d, None, None, p.id_base, p.id_stride, o_ids, o_d, o_c)
    torch.cuda.synchronize()
    assert (o_c.cpu().numpy() == K).all()
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), w_ids)
    assert np.array_equal(o_d.cpu().numpy().view(np.uint32), w_d.view(np.uint32))


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32])
def test_deleted_ids_never_come_back(kind):
    N, S = LAYOUTS["contiguous"]
    vs, lv, Q = rand_vectors(N, D, 21), O.draw_levels(N, M, 21), rand_vectors(NQ_E2E, D, 22)
    p = H.PartitionedIndex.build(vs, S, M, 32, kind, layout="contiguous", levels=lv, nb_threads=4)  # (its own: it is changed)
    before = p.search_batch(Q, K, EF)
    top1 = np.unique(before[0][:, 0])  # every query's nearest goes, and random ids up to 200
    rest = np.setdiff1d(np.arange(N, dtype=np.uint32), top1)
    gone = np.concatenate([top1, np.random.default_rng(5).choice(rest, 200 - top1.size, replace=False)]).astype(np.uint32)
    p.mark_deleted(gone)
    assert p.deleted_ids().size == 200
    got = p.search_batch(Q, K, EF)
    assert not np.isin(got[0], gone).any() and (got[2] > 0).all()
    per = [sh.search_batch(Q, K, EF) for sh in p.shards]
    want = merge_restate(np.stack([x[0] for x in per]), np.stack([x[1] for x in per]), np.stack([x[2] for x in per]),
                         np.stack([x[3] for x in per]), p.id_base, p.id_stride, K)
    assert_rows_equal(got, want, "kind %d deleted" % kind)
    p.unmark_deleted(gone)
    assert_rows_equal(p.search_batch(Q, K, EF), before, "kind %d undeleted" % kind)


# ---- 5. RCCL ---------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rccl_worker(rank, world_size, port, outdir):
    import torch
    import torch.distributed as dist
    from tests.conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world_size)
    import hnsw_rs_amd as HH
    from hnsw_rs_amd.distributed import PartitionedSearcher, make_device_merge, make_shard_search
    N = 3000
    vs, lv, Q = rand_vectors(N, D, 21), O.draw_levels(N, M, 21), rand_vectors(NQ_E2E, D, 22)
    dev = torch.device("cuda:0")
    index = HH.HNSW.new(M, 32, D, HH.VEC_F32).insert_bulk(vs, 4, False, levels=lv)  # S = 1: the one shard holds all
    ps = PartitionedSearcher(make_shard_search(index, K, EF, NQ_E2E, dev), make_device_merge(K, dev), D, K, dev, [0], [1])
    with HH.kernel_log() as log:
        got = ps.search(torch.from_numpy(Q).to(dev), NQ_E2E)
        torch.cuda.synchronize()
    ids, dists, counts, st = oracle_from_product(index, vs, lv).search_batch(Q, K, EF)
    st4 = np.concatenate([st.astype(np.int64), np.zeros((NQ_E2E, 1), dtype=np.int64)], axis=1)
    want = merge_restate(ids[None], dists[None], counts[None], st4[None], [0], [1], K)
    ok = (np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0])
          and np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
          and np.array_equal(got[2].cpu().numpy().view(np.uint32), want[2])
          and np.array_equal(got[3].cpu().numpy().astype(np.int64), want[3]))
    np.savez(os.path.join(outdir, "rccl.npz"), ok=np.array([int(ok)]), merges=np.array([log.get("hx_filt_merge_kernel", 0)]))
    dist.barrier()
    dist.destroy_process_group()


def test_partitioned_searcher_on_a_one_rank_rccl_communicator(tmp_path):
    """backend nccl IS RCCL on ROCm: the broadcast and the four gathers run through it on device buffers (a communicator
    of one rank: the same calls, no peer), then the HIP merge reads the gathered [W][nq][...] buffers as they are"""
    import torch.multiprocessing as mp
    mp.spawn(_rccl_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    r = np.load(tmp_path / "rccl.npz")
    assert r["merges"][0] == 1
    assert r["ok"][0] == 1, "the partitioned search over nccl differs from the oracle's search merged by the restatement"
