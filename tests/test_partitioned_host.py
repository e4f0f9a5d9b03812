"""Partitioned search on the host (include/hnsw_mi355x.h, "partitioned search"): the two prototypes against the ctypes
binding, every argument error hnsw_merge_topk_device and hnsw_search_batch_shards decide before they touch a device,
PartitionedIndex's id maps, build, save / load and deletion routing, the numpy restatement of the merge against a brute
sort, and PartitionedSearcher over world-size-2 gloo with the CPU oracle as the shards' search.  None of this needs a GPU."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.conftest import ROOT
from tests.partitioned_restate import merge_restate
from tests.util import rand_vectors

MAX = 0xFFFFFFFF
D = 12
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
NEW_SYMBOLS = ("hnsw_merge_topk_device", "hnsw_search_batch_shards")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=300, kind=H.VEC_QUANT8, seed=1, d=D):
    return H.HNSW.new(8, 32, d, kind).insert_bulk(rand_vectors(n, d, seed), 2, False, levels=O.draw_levels(n, 8, seed))


# ---- ABI ----------------------------------------------------------------------------------------------------------
def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers and the stream: void
    pointers, passed as integers; the array of handles: a pointer to void pointers)"""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if kind == "hnsw_index**":
        return C.POINTER(C.c_void_p)
    if name.startswith("d_") or kind == "void*":
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int
        assert [c_type_of(p) for p in params] == argtypes, name
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 14 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 12
    assert re.search(r"#define HNSW_MERGE_MAX_SHARDS 64\b", header)
    for name in ("PartitionedIndex", "merge_topk"):
        assert hasattr(H, name), name
    for key in ("shard_calls", "shard_merges"):
        assert small(n=50).stat(key) == 0


# ---- argument errors: decided before the device is touched ----------------------------------------------------------
def test_merge_argument_errors_need_no_device():
    L = _lib.lib()
    base, stride = np.arange(4, dtype=np.uint32), np.full(4, 4, dtype=np.uint32)
    fake = 0x10000  # never dereferenced: every call below is refused (or has nothing to do) on the host

    def rc(**kw):
        a = dict(S=4, nq=8, n=10, ids_in=fake, dists_in=fake, counts_in=fake, stats_in=fake, base=base, stride=stride,
                 ids=fake, dists=fake, counts=fake, stats=fake)
        a.update(kw)
        return L.hnsw_merge_topk_device(a["S"], a["nq"], a["n"], a["ids_in"], a["dists_in"], a["counts_in"], a["stats_in"],
                                        ptr(a["base"], u32p), ptr(a["stride"], u32p), a["ids"], a["dists"], a["counts"],
                                        a["stats"], None)

    for S in (0, 65, 1000):
        big = np.zeros(max(S, 1), dtype=np.uint32)
        assert rc(S=S, base=big, stride=big) == _lib.ERR_ARG, S
    assert b"shards" in L.hnsw_last_error()
    for n in (0, 65, MAX):
        assert rc(n=n) == _lib.ERR_ARG, n
    assert rc(nq=1 << 31) == _lib.ERR_ARG and rc(nq=(1 << 40) + 1) == _lib.ERR_ARG
    for name in ("ids_in", "dists_in", "base", "ids", "dists"):
        assert rc(**{name: None}) == _lib.ERR_ARG, name
    assert rc(stats_in=None) == _lib.ERR_ARG and rc(stats=None) == _lib.ERR_ARG  # exactly one of the two
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0: HNSW_OK and no launch, whatever else is passed
    assert rc(nq=0) == _lib.OK
    assert rc(nq=0, S=0, n=0, ids_in=None, dists_in=None, base=None, stride=None, ids=None, dists=None, stats=None) == _lib.OK
    with pytest.raises(ValueError):
        H.merge_topk(4, 8, 10, fake, fake, None, None, [0, 1, 2], None, fake, fake)  # one base per shard
    with pytest.raises(ValueError):
        H.merge_topk(2, 8, 10, fake, fake, None, None, [0, -1], None, fake, fake)


def test_shards_argument_errors_need_no_device():
    L = _lib.lib()
    a, b = small(seed=1), small(seed=2)
    other_dim = small(seed=3, d=D + 1)
    empty = H.HNSW.new(8, 32, D, H.VEC_QUANT8)
    Q = rand_vectors(5, D, 9)
    base = np.array([0, 300], dtype=np.uint32)

    def rc(shards=(a, b), n_shards=None, base=base, stride=None, Q=Q, nq=5, n=4, ef=16, ids="own", counts=None):
        hs = (C.c_void_p * max(len(shards), 1))(*[None if s is None else s._h.value for s in shards])
        out = np.full((5, max(min(n, 64), 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        dists = np.full((5, max(min(n, 64), 1)), 3.5, dtype=np.float32)
        code = L.hnsw_search_batch_shards(hs, len(shards) if n_shards is None else n_shards, ptr(base, u32p),
                                          ptr(stride, u32p), ptr(Q, f32p), nq, n, ef, ptr(out, u32p), ptr(dists, f32p),
                                          ptr(counts, u32p), None)
        if code != _lib.OK:  # an error leaves the outputs as they were
            assert (dists == 3.5).all() and (out is None or (out == 7).all())
        return code

    before = {k: a.stat(k) for k in ("uploads", "shard_calls", "shard_merges")}
    assert L.hnsw_search_batch_shards(None, 2, ptr(base, u32p), None, ptr(Q, f32p), 5, 4, 16, None, None, None, None) == _lib.ERR_ARG
    assert rc(n_shards=0) == _lib.ERR_ARG and rc(n_shards=65) == _lib.ERR_ARG
    assert rc(base=None) == _lib.ERR_ARG
    assert rc(shards=(a, None)) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    assert rc(shards=(a, other_dim)) == _lib.ERR_ARG
    assert b"dimension" in L.hnsw_last_error()
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(nq=1 << 31) == _lib.ERR_ARG
    assert rc(Q=None) == _lib.ERR_ARG and rc(ids=None) == _lib.ERR_ARG
    assert rc(shards=(a, empty)) == _lib.ERR_EMPTY
    a.set_device(0)
    b.set_device(1)
    assert rc() == _lib.ERR_ARG
    assert b"device" in L.hnsw_last_error()
    b.set_device(0)
    # nq == 0 is HNSW_OK; n == 0 zeroes the counts and launches nothing
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None) == _lib.OK
    counts = np.full(5, 9, dtype=np.uint32)
    assert rc(n=0, counts=counts) == _lib.OK and (counts == 0).all()
    assert {k: a.stat(k) for k in before} == before


# ---- id maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_id_maps_round_trip_over_uneven_shards(layout):
    from hnsw_rs_amd.partitioned import partition_rows
    N, S = 3001, 4
    rows, base, stride = partition_rows(N, S, layout)
    sizes = [len(range(*r.indices(N))) for r in rows]
    assert sum(sizes) == N and (sizes == [751, 751, 751, 748] if layout == "contiguous" else sizes == [751, 750, 750, 750])
    if layout == "contiguous":
        assert base.tolist() == [0, 751, 1502, 2253] and stride.tolist() == [1, 1, 1, 1]
    else:
        assert base.tolist() == [0, 1, 2, 3] and stride.tolist() == [4, 4, 4, 4]

    class Stub:  # the maps need no shard: a PartitionedIndex over stand-ins of the right count
        dim, vec_kind = D, H.VEC_F32

    p =H.PartitionedIndex([Stub() for _ in range(S)], base, stride, layout, N)
    g = np.arange(N, dtype=np.uint32)
    s, loc = p.to_local(g)
    seen = np.zeros(N, dtype=bool)
    for k in range(S):
        mine = np.arange(N)[rows[k]]
        assert np.array_equal(g[s == k], mine)  # the rows the layout gave shard k, in its local order
        assert np.array_equal(loc[s == k], np.arange(sizes[k]))
        assert np.array_equal(p.to_global(k, np.arange(sizes[k])), mine)
        seen[mine] = True
    assert seen.all()
    assert p.to_local(N - 1) == (int(s[-1]), int(loc[-1])) and p.to_global(int(s[-1]), int(loc[-1])) == N - 1


def test_build_refuses_what_the_id_space_cannot_hold():
    too_many = np.broadcast_to(np.zeros((1, 4), dtype=np.float32), (2 ** 32 - 1, 4))  # (a view: no memory behind it)
    with pytest.raises(ValueError):
        H.PartitionedIndex.build(too_many, 4, 8, 32)
    vs = rand_vectors(10, D, 1)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            H.PartitionedIndex.build(vs, bad, 8, 32)
    with pytest.raises(ValueError):
        H.PartitionedIndex.build(vs, 2, 8, 32, layout="hashed")
    with pytest.raises(ValueError):
        H.PartitionedIndex.build(vs[:3], 4, 8, 32)  # a shard would be empty


# ---- build, save / load, deletion routing -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_build_save_load_and_deletion_routing(tmp_path, layout):
    N, S = 1001, 3
    vs, lv = rand_vectors(N, D, 4), O.draw_levels(N, 8, 4)
    p = H.PartitionedIndex.build(vs, S, 8, 32, H.VEC_F32, layout=layout, levels=lv, nb_threads=1)
    assert len(p) == N and len(p.shards) == S and p.dim == D
    for k, sh in enumerate(p.shards):
        rows = np.arange(N)[k * 334:(k + 1) * 334] if layout == "contiguous" else np.arange(N)[k::S]
        assert sh.len() == rows.size
        one = H.HNSW.new(8, 32, D, H.VEC_F32).insert_bulk(vs[rows], 1, False, levels=lv[rows])  # an ordinary build
        assert np.array_equal(sh.get_point(5).get_vals(), vs[rows[5]])
        for a, b in zip(sh.iter_layers(), one.iter_layers()):
            assert all(np.array_equal(x, y) for x, y in zip(a.csr(), b.csr()))
    rng = np.random.default_rng(3)
    gone = rng.choice(N, 120, replace=False).astype(np.uint32)
    p.mark_deleted(gone)
    s_of, loc = p.to_local(gone)
    for k, sh in enumerate(p.shards):
        assert np.array_equal(sh.deleted_ids(), np.sort(loc[s_of == k]))
    assert np.array_equal(p.deleted_ids(), np.sort(gone))
    p.unmark_deleted(gone[:50])
    assert np.array_equal(p.deleted_ids(), np.sort(gone[50:]))
    with pytest.raises(H.HnswError):
        p.mark_deleted([0, N])  # an id the index does not have: nothing changes
    assert np.array_equal(p.deleted_ids(), np.sort(gone[50:]))
    p.save(tmp_path / "part")
    assert sorted(os.listdir(tmp_path / "part")) == ["partition.json", "shard_0", "shard_1", "shard_2"]
    q = H.PartitionedIndex.load(tmp_path / "part")
    assert q.layout == layout and len(q) == N and q.n_points == N
    assert np.array_equal(q.id_base, p.id_base) and np.array_equal(q.id_stride, p.id_stride)
    assert np.array_equal(q.deleted_ids(), p.deleted_ids())
    for a, b in zip(p.shards, q.shards):
        assert a.len() == b.len() and a.nb_layers() == b.nb_layers() and int(a.params.ep) == int(b.params.ep)
        for la, lb in zip(a.iter_layers(), b.iter_layers()):
            assert all(np.array_equal(x, y) for x, y in zip(la.csr(), lb.csr()))
    g = np.arange(N)
    assert all(np.array_equal(x, y) for x, y in zip(p.to_local(g), q.to_local(g)))


# ---- the restatement against a brute sort --------------------------------------------------------------------------
def brute_merge(ids, dists, counts, stats, base, stride, n):
    """the definition, entry by entry in plain Python"""
    S, nq, _ = ids.shape
    out = []
    for q in range(nq):
        status = 0
        for s in range(S):
            if stats is not None and status == 0:
                status = int(stats[s, q, 3])
        pairs = set()
        for s in range(S):
            for j in range(n):
                here = j < min(int(counts[s, q]), n) if counts is not None else int(ids[s, q, j]) != MAX
                if here:
                    bits = int(np.float32(dists[s, q, j]).view(np.uint32))
                    pairs.add((bits, int(base[s]) + int(stride[s]) * int(ids[s, q, j])))
        top = [] if status else sorted(pairs)[:n]
        sums = [int(sum(int(stats[s, q, c]) for s in range(S)) % 2 ** 32) for c in range(3)] if stats is not None else None
        out.append((top, status, sums))
    return out


@pytest.mark.parametrize("with_counts", [True, False])
def test_restatement_is_the_definition(with_counts):
    rng = np.random.default_rng(11)
    S, nq, n = 5, 23, 7
    ids = rng.integers(0, 40, (S, nq, n)).astype(np.uint32)  # few ids, few distances: equal pairs across shards
    dists = (rng.integers(0, 6, (S, nq, n)) * 0.25).astype(np.float32)
    counts = rng.integers(0, n + 3, (S, nq)).astype(np.uint32)  # (beyond n: clamped)
    if not with_counts:
        ids[rng.random((S, nq, n)) < 0.3] = MAX
    stats = rng.integers(0, 2 ** 32, (S, nq, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    stats[3, 4, 3], stats[1, 4, 3], stats[2, 9, 3] = -2, -11, -3
    base, stride = np.array([0, 3, 10, 0, 1000], dtype=np.uint32), np.array([1, 1, 2, 1, 7], dtype=np.uint32)
    got = merge_restate(ids, dists, counts if with_counts else None, stats, base, stride, n)
    want = brute_merge(ids, dists, counts if with_counts else None, stats, base, stride, n)
    assert got[3][4, 3] == -11 and got[3][9, 3] == -3 and got[2][4] == 0 and got[2][9] == 0
    for q, (top, status, sums) in enumerate(want):
        assert got[2][q] == len(top) and got[3][q, 3] == status and got[3][q, :3].tolist() == sums
        assert got[0][q, :len(top)].tolist() == [t[1] for t in top]
        assert got[1][q, :len(top)].view(np.uint32).tolist() == [t[0] for t in top]
        assert (got[0][q, len(top):] == MAX).all() and np.isposinf(got[1][q, len(top):]).all()
    assert merge_restate(ids, dists, None, None, base, None, n)[3] is None


# ---- PartitionedSearcher over gloo ------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO_N, GLOO_NQ, GLOO_K, GLOO_EF, GLOO_M = 801, 37, 5, 20, 8


def _gloo_shard_search(rank, world, vs, lv):
    """the CPU oracle over shard `rank` of the strided layout -> a search in numpy"""
    rows = np.arange(GLOO_N)[rank::world]
    orc = O.OracleHNSW(GLOO_M, None, D).insert_bulk(vs[rows], lv[rows])

    def search(Q):
        ids, dists, counts, st = orc.search_batch(Q, GLOO_K, GLOO_EF)
        return ids, dists, counts, np.concatenate([st.astype(np.int64), np.zeros((len(Q), 1), dtype=np.int64)], axis=1)

    return search


def _gloo_worker(rank, world, port, outfile, inject):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hnsw_rs_amd.distributed import PartitionedSearcher
    vs, lv = rand_vectors(GLOO_N, D, 1), O.draw_levels(GLOO_N, GLOO_M, 1)
    search = _gloo_shard_search(rank, world, vs, lv)
    base, stride = list(range(world)), [world] * world

    def local_search(Q):
        if inject == "raise" and rank == 1:
            raise H.HnswError(_lib.ERR_HIP, "injected")
        ids, dists, counts, st = search(Q.numpy())
        if inject == "status" and rank == 1:
            st[6, 3] = _lib.ERR_NAN_INPUT
        return (torch.from_numpy(ids.view(np.int32)), torch.from_numpy(dists), torch.from_numpy(counts.view(np.int32)),
                torch.from_numpy(st.astype(np.int32)))

    def merge(ids, dists, counts, stats, b, s):
        o = merge_restate(ids.numpy().view(np.uint32), dists.numpy(), counts.numpy().view(np.uint32), stats.numpy(), b, s,
                          GLOO_K)
        return (torch.from_numpy(o[0].view(np.int32)), torch.from_numpy(o[1]), torch.from_numpy(o[2].view(np.int32)),
                torch.from_numpy(o[3].astype(np.int32)))

    ps = PartitionedSearcher(local_search, merge, D, GLOO_K, torch.device("cpu"), base, stride)
    Qn = rand_vectors(GLOO_NQ, D, 2)
    verdict = "?"
    try:
        got = ps.search(torch.from_numpy(Qn) if rank == 0 else None, GLOO_NQ)
        if rank == 0:
            # the restatement applied directly to what every shard's search returns
            per = [_gloo_shard_search(r, world, vs, lv)(Qn) for r in range(world)]
            want = merge_restate(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]),
                                 np.stack([p[3] for p in per]), base, stride, GLOO_K)
            ok = (np.array_equal(got[0].numpy().view(np.uint32), want[0])
                  and np.array_equal(got[1].numpy().view(np.uint32), want[1].view(np.uint32))
                  and np.array_equal(got[2].numpy().view(np.uint32), want[2])
                  and np.array_equal(got[3].numpy().astype(np.int64), want[3])
                  and (want[2] == GLOO_K).all() and len(set(want[0][0] % world)) > 1)  # (both shards contribute)
            verdict = "ok" if ok else "mismatch"
        else:
            verdict = "ok" if got == (None, None, None, None) else "mismatch"
    except RuntimeError as e:
        verdict = "raised: %s" % e
    open(outfile + ".%d" % rank, "w").write(verdict)
    dist.barrier()  # every rank is still in step: nobody hangs in a collective the other never enters
    dist.destroy_process_group()


@pytest.mark.parametrize("inject", [None, "status", "raise"])
def test_partitioned_searcher_world_size_2_gloo(tmp_path, inject):
    import torch.multiprocessing as mp
    out = str(tmp_path / "verdict")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out, inject), nprocs=2, join=True)
    root, other = open(out + ".0").read(), open(out + ".1").read()
    if inject is None:
        assert root == "ok" and other == "ok"
    elif inject == "status":  # one query failed on the non-root rank: the root raises after the gathers, naming it
        assert root.startswith("raised") and "query 6" in root and "status -2" in root, root
        assert other == "ok"
    else:  # the non-root rank's search failed outright: it raises after its last gather, the root after the merge
        assert root.startswith("raised") and "query 0" in root and "status -5" in root, root
        assert other.startswith("raised") and "injected" in other, other
