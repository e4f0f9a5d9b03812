"""Partitioned search (include/hnsw_mi355x.h, "partitioned search"): one index cut into S shards, each an ordinary
HNSW with ids local to it; every shard answers every query and the S result lists of a query are merged on the device
into its n best by (distance bits, global id).

    merge_topk(...)        hnsw_merge_topk_device: the merge alone, over device pointers, one kernel launch
    PartitionedIndex       S shards on one GPU answered as one index (hnsw_search_batch_shards), with the id maps,
                           deletion routed to the shards, save / load

One shard per rank over RCCL is hnsw_rs_amd.distributed.PartitionedSearcher.  Global id = id_base[s] + id_stride[s] *
local id: "contiguous" gives shard s the block of ceil(N / S) rows from s * ceil(N / S), "strided" the rows s, s + S, ...
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from ._lib import HnswError, QueryStats, check
from .hnsw import HNSW

MAX_SHARDS = 64  # HNSW_MERGE_MAX_SHARDS
_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)


def _dptr(t):
    """a torch device tensor (or a raw device pointer, or None) -> the pointer as an int or None"""
    if t is None or isinstance(t, (int, np.integer)):
        return int(t) if t else None
    return t.data_ptr()


def _u32(a, what):
    a = np.asarray(a).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > _lib.UINT32_MAX):
        raise ValueError("%s must be in [0, 2^32)" % what)
    return np.ascontiguousarray(a, dtype=np.uint32)


def merge_topk(n_shards, nq, n, d_ids_in, d_dists_in, d_counts_in, d_stats_in, id_base, id_stride, d_ids, d_dists,
               d_counts=None, d_stats=None, stream=0):
    """hnsw_merge_topk_device over torch device tensors (or raw device pointers): the [S][nq][n] ids / dists (and
    [S][nq] counts / stats, or None) of S shards -> the n best of every query by (distance bits, id_base[s] +
    id_stride[s] * local id), duplicates dropped, in d_ids / d_dists (/ d_counts / d_stats).  ONE launch enqueued on
    `stream`, on the current device; nothing is allocated, copied or synchronised.  id_base / id_stride are host
    arrays (id_stride None: all 1); the caller guarantees that no global id reaches UINT32_MAX."""
    base = _u32(id_base, "id_base")
    stride = None if id_stride is None else _u32(id_stride, "id_stride")
    if base.shape[0] != n_shards or (stride is not None and stride.shape[0] != n_shards):
        raise ValueError("id_base / id_stride need one entry per shard")
    p = _dptr
    check(_lib.lib().hnsw_merge_topk_device(
        n_shards, nq, n, p(d_ids_in), p(d_dists_in), p(d_counts_in), p(d_stats_in), base.ctypes.data_as(_u32p),
        None if stride is None else stride.ctypes.data_as(_u32p), p(d_ids), p(d_dists), p(d_counts), p(d_stats),
        stream or None))


def partition_rows(n_points, n_shards, layout):
    """-> (rows per shard as slices of range(n_points), id_base, id_stride) of a layout"""
    if not 1 <= n_shards <= MAX_SHARDS:
        raise ValueError("1 to %d shards" % MAX_SHARDS)
    if n_points >= _lib.UINT32_MAX:
        raise ValueError("a partitioned index holds fewer than 2^32 - 1 points (ids are uint32, UINT32_MAX pads)")
    if layout == "contiguous":
        per = (n_points + n_shards - 1) // n_shards
        rows = [slice(min(n_points, s * per), min(n_points, (s + 1) * per)) for s in range(n_shards)]
        base, stride = [s * per for s in range(n_shards)], [1] * n_shards
    elif layout == "strided":
        rows = [slice(s, n_points, n_shards) for s in range(n_shards)]
        base, stride = list(range(n_shards)), [n_shards] * n_shards
    else:
        raise ValueError("layout is 'contiguous' or 'strided'")
    if any(len(range(*r.indices(n_points))) == 0 for r in rows):
        raise ValueError("%d points leave a shard of %d empty (%s)" % (n_points, n_shards, layout))
    return rows, np.array(base, dtype=np.uint32), np.array(stride, dtype=np.uint32)


class PartitionedIndex:
    """S ordinary indexes on one GPU answered as one.  .shards (HNSW), .id_base / .id_stride (uint32 [S]), .layout."""

    def __init__(self, shards, id_base, id_stride, layout, n_points):
        self.shards = list(shards)
        self.id_base = _u32(id_base, "id_base")
        self.id_stride = _u32(id_stride, "id_stride")
        self.layout, self.n_points = layout, int(n_points)
        if not (len(self.shards) == self.id_base.shape[0] == self.id_stride.shape[0]) or not self.shards:
            raise ValueError("one id_base and one id_stride per shard")
        self.dim, self.vec_kind = self.shards[0].dim, self.shards[0].vec_kind
        # (contiguous: the block length the map divides by)
        self._per = (self.n_points + len(self.shards) - 1) // len(self.shards)

    @staticmethod
    def build(vectors, n_shards, m, ef_cons, vec_kind=_lib.VEC_QUANT8, layout="contiguous", levels=None, nb_threads=8):
        """S ordinary builds (HNSW.insert_bulk), one per shard, over the rows the layout gives it; levels: the level
        of every row of `vectors`, or None (drawn per shard)."""
        n_points = len(vectors)
        rows, base, stride = partition_rows(n_points, n_shards, layout)  # (refuses N >= 2^32 - 1 before a row is read)
        vs = np.ascontiguousarray(vectors, dtype=np.float32)
        if vs.ndim != 2:
            raise HnswError(_lib.ERR_BAD_DIM, "vectors must be N x dim")
        lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        if lv is not None and lv.shape[0] != n_points:
            raise HnswError(_lib.ERR_ARG, "levels and vectors differ in length")
        shards = [HNSW.new(m, ef_cons, vs.shape[1], vec_kind).insert_bulk(vs[r], nb_threads, False,
                                                                          levels=None if lv is None else lv[r])
                  for r in rows]
        return PartitionedIndex(shards, base, stride, layout, n_points)

    def len(self):
        return sum(s.len() for s in self.shards)

    def __len__(self):
        return self.len()

    # ---- id maps ---------------------------------------------------------------------------------------------------
    def to_global(self, s, local):
        """local id(s) of shard s -> global id(s)"""
        loc = np.asarray(local, dtype=np.uint64)
        g = np.uint64(self.id_base[s]) + np.uint64(self.id_stride[s]) * loc
        return g.astype(np.uint32) if g.ndim else int(g)

    def to_local(self, global_ids):
        """global id(s) -> (shard, local id); arrays for an array"""
        g = np.asarray(global_ids, dtype=np.uint64)
        if self.layout == "contiguous":
            s, loc = g // np.uint64(self._per), g % np.uint64(self._per)
        else:
            S = np.uint64(len(self.shards))
            s, loc = g % S, g // S
        if g.ndim:
            return s.astype(np.int64), loc.astype(np.uint32)
        return int(s), int(loc)

    # ---- query -----------------------------------------------------------------------------------------------------
    def search_batch(self, Q, n, ef):
        """hnsw_search_batch_shards -> ids [nq, n] GLOBAL (pad UINT32_MAX), dists [nq, n], counts [nq], stats [nq, 4]
        (n_dist, n_exp, sum_deg summed over the shards; status)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq, S = Q.shape[0], len(self.shards)
        ids = np.full((nq, max(n, 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(n, 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        handles = (C.c_void_p * S)(*[s._h.value for s in self.shards])
        check(_lib.lib().hnsw_search_batch_shards(
            handles, S, self.id_base.ctypes.data_as(_u32p), self.id_stride.ctypes.data_as(_u32p),
            Q.ctypes.data_as(_f32p), nq, n, ef, ids.ctypes.data_as(_u32p), dists.ctypes.data_as(_f32p),
            counts.ctypes.data_as(_u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids[:, :n], dists[:, :n], counts, stats.view(np.uint32).astype(np.int64)

    # ---- deletion, routed to the shards ----------------------------------------------------------------------------
    def _route(self, global_ids):
        g = _u32(global_ids, "ids")
        if g.size and int(g.max()) >= self.n_points:
            raise HnswError(_lib.ERR_ARG, "id %d is not below the %d points of the index" % (int(g.max()), self.n_points))
        s, loc = self.to_local(g)
        return [(k, loc[s == k]) for k in range(len(self.shards)) if (s == k).any()]

    def mark_deleted(self, global_ids):
        """HNSW.mark_deleted on the shard of every id (an id >= len: HnswError, nothing changes)"""
        for k, loc in self._route(global_ids):
            self.shards[k].mark_deleted(loc)

    def unmark_deleted(self, global_ids):
        for k, loc in self._route(global_ids):
            self.shards[k].unmark_deleted(loc)

    def deleted_ids(self):
        """-> the deleted global ids, ascending"""
        parts = [self.to_global(k, s.deleted_ids()) for k, s in enumerate(self.shards)]
        return np.sort(np.concatenate(parts)).astype(np.uint32)

    # ---- persistence -----------------------------------------------------------------------------------------------
    def save(self, path):
        """shard_<k>/ through HNSW.save, and partition.json: layout, S, bases and strides"""
        path = str(path)
        os.makedirs(path, exist_ok=True)
        for k, s in enumerate(self.shards):
            s.save(os.path.join(path, "shard_%d" % k))
        with open(os.path.join(path, "partition.json"), "w") as f:
            json.dump({"layout": self.layout, "n_shards": len(self.shards), "n_points": self.n_points,
                       "id_base": [int(x) for x in self.id_base], "id_stride": [int(x) for x in self.id_stride]}, f)

    @staticmethod
    def load(path):
        path = str(path)
        with open(os.path.join(path, "partition.json")) as f:
            meta = json.load(f)
        shards = [HNSW.load(os.path.join(path, "shard_%d" % k)) for k in range(int(meta["n_shards"]))]
        return PartitionedIndex(shards, meta["id_base"], meta["id_stride"], meta["layout"], meta["n_points"])
