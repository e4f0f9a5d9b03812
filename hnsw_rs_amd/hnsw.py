"""Host-side mirror of the reference's `hnsw::template::HNSW` (hnsw/src/template.rs) on top of the
C ABI of libhnsw_mi355x.so.  Same method names, argument meaning and error behaviour as the Rust
API, so that the parity tests read like the reference's own tests; the search itself runs in the
HIP kernels behind `hnsw_search_batch*` (there is no Python / CPU search path).

    index = HNSW.new(12, None, dim)                    # template.rs:133
    index = index.insert_bulk(vectors, 1, False)       # template.rs:388 (returns the index)
    node = index.insert_vec(vector)                    # template.rs:165
    ids = index.ann_by_vector(query, 10, 100)          # template.rs:306
    index.save(path); index = HNSW.load(path)          # template.rs:43,75
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VEC_F32, VEC_QUANT8, HnswError, Params, QueryStats, check

_f32p, _u8p, _u32p, _u64p = _lib.f32p, _lib.u8p, _lib.u32p, _lib.u64p


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class Point:
    """What get_point(id) exposes in the reference (points/src/point.rs:6-10)."""

    def __init__(self, index, node):
        self._index, self.id = index, node
        lv = C.c_uint32()
        check(index._L.hnsw_get_level(index._h, node, C.byref(lv)))
        self.level = lv.value

    def get_vals(self):  # VecBase::get_vals, vectors/src/lib.rs:24-26
        out = np.zeros(self._index.dim, dtype=np.float32)
        check(self._index._L.hnsw_get_vector(self._index._h, self.id, _p(out, _f32p)))
        return out

    def quant(self):
        """(min, delta, codes) of the stored QuantVec (vectors/src/quant.rs:6-11)"""
        codes = np.zeros(self._index.dim, dtype=np.uint8)
        mn, dl = C.c_float(), C.c_float()
        check(self._index._L.hnsw_get_quant(self._index._h, self.id, _p(codes, _u8p), C.byref(mn),
                                            C.byref(dl)))
        return np.float32(mn.value), np.float32(dl.value), codes


class Graph:
    """Read-only view of one layer (graph/src/graph.rs:9-16)."""

    def __init__(self, index, level):
        self._index, self.level = index, level
        self.m = int(index._L.hnsw_layer_m(index._h, level))

    def nb_nodes(self):
        return int(self._index._L.hnsw_layer_nb_nodes(self._index._h, self.level))

    def iter_nodes(self):
        n = self.nb_nodes()
        out = np.zeros(max(n, 1), dtype=np.uint32)
        cnt = C.c_uint64()
        check(self._index._L.hnsw_layer_nodes(self._index._h, self.level, _p(out, _u32p), n, C.byref(cnt)))
        return out[:n]

    def neighbors(self, node):  # Err(NodeNotInGraph) -> HnswError
        buf = np.zeros(1024, dtype=np.uint32)
        deg = C.c_uint32()
        check(self._index._L.hnsw_neighbors(self._index._h, self.level, int(node), _p(buf, _u32p), 1024,
                                            C.byref(deg)))
        return set(int(x) for x in buf[: deg.value])

    def neighbors_vec(self, node):
        return sorted(self.neighbors(node))

    def degree(self, node):
        deg = C.c_uint32()
        check(self._index._L.hnsw_neighbors(self._index._h, self.level, int(node), None, 0, C.byref(deg)))
        return deg.value

    def contains(self, node):
        try:
            self.degree(node)
            return True
        except HnswError:
            return False

    def csr(self):
        """(node ids ascending, offsets u64, neighbour ids ascending per row)"""
        nn, nnz = C.c_uint64(), C.c_uint64()
        L, h = self._index._L, self._index._h
        check(L.hnsw_export_layer(h, self.level, None, None, None, C.byref(nn), C.byref(nnz)))
        ids = np.zeros(nn.value, dtype=np.uint32)
        offs = np.zeros(nn.value + 1, dtype=np.uint64)
        nbrs = np.zeros(max(nnz.value, 1), dtype=np.uint32)
        check(L.hnsw_export_layer(h, self.level, _p(ids, _u32p), _p(offs, _u64p), _p(nbrs, _u32p),
                                  C.byref(nn), C.byref(nnz)))
        return ids, offs, nbrs[: nnz.value]


class HNSW:
    def __init__(self, handle, dim, vec_kind):
        self._L = _lib.lib()
        self._h = handle
        self.dim = dim
        self.vec_kind = vec_kind

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.hnsw_free(self._h)
            self._h = None

    # ---- construction -----------------------------------------------------------------------
    @staticmethod
    def new(m, ef_cons, dim, vec_kind=VEC_QUANT8):
        """HNSW::new(m, ef_cons: Option<usize>, dim), template.rs:133-144"""
        L = _lib.lib()
        h = C.c_void_p()
        check(L.hnsw_create(m, ef_cons or 0, dim, vec_kind, C.byref(h)))
        return HNSW(h, dim, vec_kind)

    def clone(self):
        h = C.c_void_p()
        check(self._L.hnsw_clone(self._h, C.byref(h)))
        return HNSW(h, self.dim, self.vec_kind)

    @property
    def params(self):
        p = Params()
        check(self._L.hnsw_get_params(self._h, C.byref(p)))
        return p

    def set_ep(self, ep):
        check(self._L.hnsw_set_ep(self._h, int(ep)))

    def _rows(self, vectors):
        """Vec<Vec<f32>> -> n x dim float32; a row of another length is the reference's
        dimension-mismatch panic (template.rs:253-262)."""
        if isinstance(vectors, np.ndarray):
            a = np.ascontiguousarray(vectors, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != self.dim:
                raise HnswError(_lib.ERR_BAD_DIM,
                                "The current index dimension is %d, but tried inserting points of "
                                "dimension %s" % (self.dim, a.shape[1:] and a.shape[1]))
            return a
        for v in vectors:
            if len(v) != self.dim:
                raise HnswError(_lib.ERR_BAD_DIM,
                                "The current index dimension is %d, but tried inserting points of "
                                "dimension %d" % (self.dim, len(v)))
        return np.ascontiguousarray(np.array(vectors, dtype=np.float32).reshape(-1, self.dim))

    # ---- build --------------------------------------------------------------------------------
    def insert_bulk(self, vectors, nb_threads, verbose, levels=None):
        """HNSW::insert_bulk(self, vectors, nb_threads, verbose) -> Result<HNSW, String>"""
        rows = self._rows(vectors)
        lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        if lv is not None and lv.shape[0] != rows.shape[0]:
            raise HnswError(_lib.ERR_ARG, "levels and vectors differ in length")
        check(self._L.hnsw_insert_bulk_levels(self._h, _p(rows, _f32p), rows.shape[0], nb_threads,
                                              1 if verbose else 0, _p(lv, _u8p)))
        return self

    def insert_bulk_device(self, vectors, nb_threads, verbose, levels=None):
        """insert_bulk with the insertion searches + heuristic on the GPU (on-device build)"""
        rows = self._rows(vectors)
        lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        check(self._L.hnsw_insert_bulk_device(self._h, _p(rows, _f32p), rows.shape[0], nb_threads,
                                              1 if verbose else 0, _p(lv, _u8p)))
        return self

    def insert_bulk_sharded(self, vectors, nb_threads, verbose, levels=None, group=None, device=None):
        """The on-device build sharded over the ranks of a torch.distributed group (BASELINE configs[4]):
        every rank passes the same vectors / levels and ends with an identical replica; the insertion
        searches of each batch are split over the ranks by position, the connect / prune / drop phases by row
        ownership; edge records, removals and changed rows travel through all-gathers of the size the batch needs
        (RCCL when the group's backend is nccl; staged through the host for gloo)."""
        import torch
        import torch.distributed as dist
        from ._lib import ALLGATHER_FN
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        slot = int(self._L.hnsw_sharded_slot_bytes(self._h, world))
        send = torch.zeros(slot, dtype=torch.uint8, device=dev)
        recv = torch.zeros(world * slot, dtype=torch.uint8, device=dev)
        on_device = dist.get_backend(group) == "nccl"
        failure = []

        def allgather(_ctx, nbytes):
            try:
                if nbytes > slot or nbytes <= 0:
                    return 1
                # the first nbytes of every rank's send buffer, rank r's at r * nbytes of the receive buffer
                if on_device:
                    dist.all_gather_into_tensor(recv[: world * nbytes], send[:nbytes], group=group)
                    torch.cuda.synchronize(dev)
                else:  # gloo: CPU tensors
                    parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
                    dist.all_gather(parts, send[:nbytes].cpu(), group=group)
                    recv[: world * nbytes].copy_(torch.cat(parts))
                    torch.cuda.synchronize(dev)
                return 0
            except Exception as e:  # never unwind through the C frames
                failure.append(e)
                return 2

        cb = ALLGATHER_FN(allgather)
        rows = self._rows(vectors)
        lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        rc = self._L.hnsw_insert_bulk_sharded(self._h, _p(rows, _f32p), rows.shape[0], nb_threads,
                                              1 if verbose else 0, _p(lv, _u8p), rank, world,
                                              C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), slot, cb, None)
        if failure:
            raise failure[0]
        check(rc)
        return self

    def insert_vec(self, vector, level=None):
        """HNSW::insert_vec(&mut self, &Vec<f32>) -> Result<NodeID, String>"""
        v = self._rows([vector] if not isinstance(vector, np.ndarray) else vector.reshape(1, -1))
        out = C.c_uint32()
        check(self._L.hnsw_insert_vec_level(self._h, _p(v, _f32p), -1 if level is None else int(level),
                                            C.byref(out)))
        return out.value

    def import_points(self, vectors, levels):
        rows = self._rows(vectors)
        lv = np.ascontiguousarray(levels, dtype=np.uint8)
        check(self._L.hnsw_import_points(self._h, _p(rows, _f32p), rows.shape[0], _p(lv, _u8p)))

    def import_layer(self, layer, node_ids, offsets, nbrs):
        node_ids = np.ascontiguousarray(node_ids, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nbrs = np.ascontiguousarray(nbrs, dtype=np.uint32)
        check(self._L.hnsw_import_layer(self._h, layer, node_ids.shape[0], _p(node_ids, _u32p),
                                        _p(offsets, _u64p), _p(nbrs, _u32p)))

    # ---- query (GPU) ----------------------------------------------------------------------------
    def ann_by_vector(self, vector, n, ef):
        """HNSW::ann_by_vector(&self, &Vec<f32>, n, ef) -> Result<Vec<NodeID>, String>"""
        q = np.ascontiguousarray(vector, dtype=np.float32).reshape(-1)
        if q.shape[0] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "query has dimension %d, index %d" % (q.shape[0], self.dim))
        ids = np.zeros(max(n, 1), dtype=np.uint32)
        cnt = C.c_uint32()
        check(self._L.hnsw_search(self._h, _p(q, _f32p), n, ef, _p(ids, _u32p), C.byref(cnt)))
        return [int(x) for x in ids[: cnt.value]]

    def search_batch(self, Q, n, ef):
        """-> ids [nq, n] (pad UINT32_MAX), dists [nq, n], counts [nq], stats [nq, 4]
        (n_dist, n_exp, sum_deg, status)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq = Q.shape[0]
        ids = np.full((nq, max(n, 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(n, 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch(self._h, _p(Q, _f32p), nq, n, ef, _p(ids, _u32p), _p(dists, _f32p),
                                        _p(counts, _u32p),
                                        C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids[:, :n], dists[:, :n], counts, stats.view(np.uint32).astype(np.int64)

    def _filtered(self, fn, Q, n, ef, middle):
        """A filtered host call: fn(handle, Q, nq, n, ef, *middle(nq), ids, dists, counts, stats, paths), where middle
        makes the entry point's own arguments once the queries are checked (uint32 / uint64 arrays go as pointers, None
        as NULL).  -> the five-tuple of search_batch_filtered"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq = Q.shape[0]
        mid = middle(nq)  # (the arrays stay alive here for the length of the call)
        args = [_p(x, _u64p if x.dtype == np.uint64 else _u32p) if isinstance(x, np.ndarray) else x for x in mid]
        ids = np.full((nq, max(n, 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(n, 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        paths = np.zeros(nq, dtype=np.uint8)
        check(fn(self._h, _p(Q, _f32p), nq, n, ef, *args, _p(ids, _u32p), _p(dists, _f32p), _p(counts, _u32p),
                 C.cast(stats.ctypes.data, C.POINTER(QueryStats)), _p(paths, _u8p)))
        return ids[:, :n], dists[:, :n], counts, stats.view(np.uint32).astype(np.int64), paths

    def _filtered_device(self, fn, d_Q, nq, n, ef, middle, d_ids, d_dists, d_counts, d_stats, stream):
        """A filtered device call: torch device tensors, raw device pointers (ints) or None / 0 for the buffers; `middle`:
        the entry point's own arguments, as they go to fn"""
        p = self._dptr
        check(fn(self._h, p(d_Q), nq, n, ef, *middle, p(d_ids), p(d_dists), p(d_counts), p(d_stats), stream or None))

    def _filtered_device_finish(self, fn, d_Q, nq, n, ef, middle, d_ids, d_dists, d_counts, d_stats, stream, paths):
        """... and its _finish.  paths=True -> uint8 [nq] (0 / 2)"""
        p = self._dptr
        out = np.zeros(nq, dtype=np.uint8) if paths else None
        check(fn(self._h, p(d_Q), nq, n, ef, *middle, p(d_ids), p(d_dists), p(d_counts), p(d_stats), stream or None,
                 None if out is None else _p(out, _u8p)))
        return out

    def search_batch_filtered(self, Q, n, ef, allow):
        """k-NN among the allowed ids (include/hnsw_mi355x.h, hnsw_search_batch_filtered).  allow: a bool array
        over ids (its length is allow_bits) or an array of allowed ids (see pack_allow).
        -> ids [nq, n] (pad UINT32_MAX), dists [nq, n], counts [nq], stats [nq, 4], paths [nq] (0 graph,
        1 exact, 2 exact after a visited-table overflow)"""
        def middle(nq):
            return pack_allow(allow, self.len())

        return self._filtered(self._L.hnsw_search_batch_filtered, Q, n, ef, middle)

    def search_batch_filtered_multi(self, Q, n, ef, masks, mask_of):
        """k-NN with an allow-list per query (include/hnsw_mi355x.h, hnsw_search_batch_filtered_multi).  masks: what
        pack_allow_many takes (None or empty when no query names a mask); mask_of [nq]: the row of masks each query
        searches under, -1 or MASK_NONE for no allow-list.  -> as search_batch_filtered"""
        def middle(nq):
            mo = self._mask_of(np.asarray(mask_of), nq)  # (required here: None is no "row 0")
            if masks is None or len(masks) == 0:
                return None, 0, 0, mo
            words, bits = pack_allow_many(masks, self.len())
            return words, words.shape[0], bits, mo

        return self._filtered(self._L.hnsw_search_batch_filtered_multi, Q, n, ef, middle)

    def mask_set(self, masks_or_n_masks, n_points=None):
        """-> MaskSet: allow-lists resident with this index (include/hnsw_mi355x.h, hnsw_mask_set).  Either what
        pack_allow_many takes (id arrays give allow_bits = n_points, default len()), or a number of empty rows of
        n_points bits (default len(); it may exceed len() to leave room for later inserts)."""
        if isinstance(masks_or_n_masks, (int, np.integer)):
            n_masks, bits, words = int(masks_or_n_masks), int(self.len() if n_points is None else n_points), None
        else:
            words, bits = pack_allow_many(masks_or_n_masks, self.len() if n_points is None else n_points)
            n_masks = words.shape[0]
        s = C.c_void_p()
        check(self._L.hnsw_mask_set_create(self._h, n_masks, bits, None if words is None or bits == 0 else _p(words, _u64p),
                                           C.byref(s)))
        return MaskSet(self, s)

    def _mask_of(self, mask_of, nq):
        if mask_of is None:
            return None
        mo = np.asarray(mask_of).reshape(-1).astype(np.int64)
        if mo.shape[0] != nq:
            raise ValueError("mask_of must hold one entry per query")
        if ((mo < -1) | (mo > _lib.MASK_NONE)).any():
            raise ValueError("mask_of entries are rows of masks, -1 or MASK_NONE")
        return np.ascontiguousarray(np.where(mo < 0, _lib.MASK_NONE, mo).astype(np.uint32))

    def search_batch_filtered_set(self, Q, n, ef, mask_set, mask_of=None):
        """search_batch_filtered_multi with the masks of a resident MaskSet (hnsw_search_batch_filtered_set): nothing
        is packed or uploaded per call.  mask_of [nq]: rows of the set, -1 or MASK_NONE; None: every query under row 0.
        -> as search_batch_filtered"""
        return self._filtered(self._L.hnsw_search_batch_filtered_set, Q, n, ef,
                              lambda nq: (mask_set._s, self._mask_of(mask_of, nq)))

    def search_batch_filtered_device(self, d_Q, nq, n, ef, mask_set, d_mask_of, d_ids, d_dists, d_counts, d_stats,
                                     stream=0):
        """hnsw_search_batch_filtered_device: raw device pointers (ints; d_mask_of 0 / None: row 0), one launch
        enqueued on `stream`, no sync."""
        self._filtered_device(self._L.hnsw_search_batch_filtered_device, d_Q, nq, n, ef,
                              (mask_set._s, self._dptr(d_mask_of)), d_ids, d_dists, d_counts, d_stats, stream)

    def search_batch_filtered_device_finish(self, d_Q, nq, n, ef, mask_set, d_mask_of, d_ids, d_dists, d_counts, d_stats,
                                            stream=0, paths=False):
        """Completes search_batch_filtered_device: synchronises, re-runs overflowed queries, answers those that fill
        the largest table by the exact path, raises the first per-query error.  paths=True -> uint8 [nq] (0 / 2)"""
        return self._filtered_device_finish(self._L.hnsw_search_batch_filtered_device_finish, d_Q, nq, n, ef,
                                            (mask_set._s, self._dptr(d_mask_of)), d_ids, d_dists, d_counts, d_stats,
                                            stream, paths)

    # ---- labels and label-range filtered search (include/hnsw_mi355x.h) ------------------------------------------
    def set_labels(self, labels, ids=None):
        """hnsw_set_labels: one uint32 label per id; ids None: labels[i] is id i's.  Every id must be < len (else
        nothing changes); an id never set has label 0.  Needs no GPU."""
        lab = self._ids(labels)
        a = None if ids is None else self._ids(ids)
        if a is not None and a.shape[0] != lab.shape[0]:
            raise ValueError("one label per id")
        check(self._L.hnsw_set_labels(self._h, None if a is None else _p(a, _u32p), _p(lab, _u32p), lab.shape[0]))

    def get_labels(self, ids=None):
        """-> the labels (uint32) of ids, or of every id 0..len-1"""
        a = None if ids is None else self._ids(ids)
        out = np.zeros(self.len() if a is None else a.shape[0], dtype=np.uint32)
        check(self._L.hnsw_get_labels(self._h, None if a is None else _p(a, _u32p), out.shape[0], _p(out, _u32p)))
        return out

    def _range(self, lo, hi, nq):
        out = []
        for x in (lo, hi):
            x = np.asarray(x)
            if x.size and (x.min() < 0 or x.max() > _lib.UINT32_MAX):
                raise ValueError("range bounds are labels: in [0, 2^32)")
            x = np.ascontiguousarray(np.broadcast_to(x.astype(np.uint32).reshape(-1), (nq,))) if x.size == 1 else \
                np.ascontiguousarray(x.reshape(-1), dtype=np.uint32)
            if x.shape[0] != nq:
                raise ValueError("lo and hi hold one entry per query (or are scalars)")
            out.append(x)
        return out

    def search_batch_filtered_range(self, Q, n, ef, lo, hi):
        """k-NN among the ids whose label lies in [lo[i], hi[i]] (hnsw_search_batch_filtered_range); scalars broadcast,
        lo > hi is an empty range.  -> as search_batch_filtered"""
        return self._filtered(self._L.hnsw_search_batch_filtered_range, Q, n, ef, lambda nq: self._range(lo, hi, nq))

    # ---- label-set filtered search: several label ranges per query ------------------------------------------------
    def search_batch_filtered_ranges(self, Q, n, ef, ranges):
        """k-NN among the ids whose label lies in at least one of the query's ranges
        (hnsw_search_batch_filtered_ranges).  ranges: one list per query, its members (lo, hi) or an int x meaning [x, x]; ragged
        lists are padded with the empty range (1, 0) (pack_ranges).  -> as search_batch_filtered"""
        def middle(nq):
            lo, hi = pack_ranges(ranges, nq)
            return lo.shape[1], lo, hi

        return self._filtered(self._L.hnsw_search_batch_filtered_ranges, Q, n, ef, middle)

    def search_batch_filtered_ranges_device(self, d_Q, nq, n, ef, n_ranges, d_lo, d_hi, d_ids, d_dists, d_counts,
                                            d_stats, stream=0):
        """hnsw_search_batch_filtered_ranges_device over torch device tensors (or raw device pointers): d_lo / d_hi
        uint32 [nq, n_ranges] in HBM; one launch enqueued on `stream`, no sync."""
        p = self._dptr
        self._filtered_device(self._L.hnsw_search_batch_filtered_ranges_device, d_Q, nq, n, ef,
                              (n_ranges, p(d_lo), p(d_hi)), d_ids, d_dists, d_counts, d_stats, stream)

    def search_batch_filtered_ranges_device_finish(self, d_Q, nq, n, ef, n_ranges, d_lo, d_hi, d_ids, d_dists, d_counts,
                                                   d_stats, stream=0, paths=False):
        """Completes search_batch_filtered_ranges_device: synchronises, re-runs overflowed queries, answers those that
        fill the largest table by the exact path, raises the first per-query error.  paths=True -> uint8 [nq] (0 / 2)"""
        p = self._dptr
        return self._filtered_device_finish(self._L.hnsw_search_batch_filtered_ranges_device_finish, d_Q, nq, n, ef,
                                            (n_ranges, p(d_lo), p(d_hi)), d_ids, d_dists, d_counts, d_stats, stream, paths)

    def count_labels_in_ranges(self, ranges):
        """hnsw_count_labels_in_ranges: the undeleted ids whose label lies in the union of `ranges` (members (lo, hi) or
        an int x meaning [x, x]) -- the planner's own count.  Needs no GPU."""
        ranges = list(ranges)
        if not ranges:
            lo = hi = np.zeros(0, dtype=np.uint32)
        else:
            lo, hi = pack_ranges([ranges], 1)
        out = C.c_uint64(0)
        check(self._L.hnsw_count_labels_in_ranges(self._h, _p(lo, _u32p) if lo.size else None,
                                                  _p(hi, _u32p) if hi.size else None, lo.size, C.byref(out)))
        return int(out.value)

    @staticmethod
    def _dptr(t):
        """a torch device tensor (or a raw device pointer, or None) -> the pointer as an int or None"""
        if t is None or isinstance(t, (int, np.integer)):
            return int(t) if t else None
        return t.data_ptr()

    def search_batch_filtered_range_device(self, d_Q, nq, n, ef, d_lo, d_hi, d_ids, d_dists, d_counts, d_stats,
                                           stream=0):
        """hnsw_search_batch_filtered_range_device over torch device tensors (or raw device pointers): d_lo / d_hi
        uint32 [nq] in HBM; one launch enqueued on `stream`, no sync."""
        p = self._dptr
        self._filtered_device(self._L.hnsw_search_batch_filtered_range_device, d_Q, nq, n, ef, (p(d_lo), p(d_hi)),
                              d_ids, d_dists, d_counts, d_stats, stream)

    def search_batch_filtered_range_device_finish(self, d_Q, nq, n, ef, d_lo, d_hi, d_ids, d_dists, d_counts, d_stats,
                                                  stream=0, paths=False):
        """Completes search_batch_filtered_range_device: synchronises, re-runs overflowed queries, answers those that
        fill the largest table by the exact path, raises the first per-query error.  paths=True -> uint8 [nq] (0 / 2)"""
        p = self._dptr
        return self._filtered_device_finish(self._L.hnsw_search_batch_filtered_range_device_finish, d_Q, nq, n, ef,
                                            (p(d_lo), p(d_hi)), d_ids, d_dists, d_counts, d_stats, stream, paths)

    # ---- a label range AND a row of a resident mask set (include/hnsw_mi355x.h) -----------------------------------
    def search_batch_filtered_set_range(self, Q, n, ef, mask_set, mask_of, lo, hi):
        """k-NN among the ids that row mask_of[i] of a resident MaskSet allows AND whose label lies in [lo[i], hi[i]]
        (hnsw_search_batch_filtered_set_range).  mask_of [nq]: rows of the set, -1 or MASK_NONE (the range alone);
        None: every query under row 0.  lo / hi: scalars broadcast, lo > hi is an empty range.
        -> as search_batch_filtered"""
        return self._filtered(self._L.hnsw_search_batch_filtered_set_range, Q, n, ef,
                              lambda nq: (mask_set._s, self._mask_of(mask_of, nq), *self._range(lo, hi, nq)))

    def search_batch_filtered_set_range_device(self, d_Q, nq, n, ef, mask_set, d_mask_of, d_lo, d_hi, d_ids, d_dists,
                                               d_counts, d_stats, stream=0):
        """hnsw_search_batch_filtered_set_range_device over torch device tensors (or raw device pointers): d_mask_of
        (None / 0: row 0), d_lo / d_hi uint32 [nq] in HBM; one launch enqueued on `stream`, no sync."""
        p = self._dptr
        self._filtered_device(self._L.hnsw_search_batch_filtered_set_range_device, d_Q, nq, n, ef,
                              (mask_set._s, p(d_mask_of), p(d_lo), p(d_hi)), d_ids, d_dists, d_counts, d_stats, stream)

    def search_batch_filtered_set_range_device_finish(self, d_Q, nq, n, ef, mask_set, d_mask_of, d_lo, d_hi, d_ids,
                                                      d_dists, d_counts, d_stats, stream=0, paths=False):
        """Completes search_batch_filtered_set_range_device: synchronises, re-runs overflowed queries, answers those
        that fill the largest table by the exact path, raises the first per-query error.
        paths=True -> uint8 [nq] (0 / 2)"""
        p = self._dptr
        return self._filtered_device_finish(self._L.hnsw_search_batch_filtered_set_range_device_finish, d_Q, nq, n, ef,
                                            (mask_set._s, p(d_mask_of), p(d_lo), p(d_hi)), d_ids, d_dists, d_counts,
                                            d_stats, stream, paths)

    # ---- grouped search: the nearest groups by label (include/hnsw_mi355x.h) ---------------------------------------
    def search_batch_grouped(self, Q, n_groups, per_group, pool, ef, mask_set=None, mask_of=None, lo=None, hi=None):
        """The n_groups nearest labels of every query with their per_group best hits each, out of the `pool` candidates
        that search_batch (or, with mask_set / lo and hi, the filtered search of that kind) returns with n = pool
        (hnsw_search_batch_grouped).  mask_of [nq]: rows of the set, -1 or MASK_NONE; None: row 0.  lo / hi: both or
        neither, scalars broadcast.
        -> ids [nq, n_groups, per_group] (pad UINT32_MAX), dists [nq, n_groups, per_group] (pad +inf), group_labels
        [nq, n_groups], group_sizes [nq, n_groups], counts [nq] (groups found), stats [nq, 4] (the candidate call's)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        if (lo is None) != (hi is None):
            raise ValueError("a label range needs lo and hi, both or neither")
        nq, G, P = Q.shape[0], max(int(n_groups), 1), max(int(per_group), 1)
        mo = self._mask_of(mask_of, nq)
        rng = (None, None) if lo is None else self._range(lo, hi, nq)
        ids = np.full((nq, G, P), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, G, P), np.inf, dtype=np.float32)
        labels = np.zeros((nq, G), dtype=np.uint32)
        sizes = np.zeros((nq, G), dtype=np.uint32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_grouped(
            self._h, _p(Q, _f32p), nq, n_groups, per_group, pool, ef, mask_set._s if mask_set is not None else None,
            None if mo is None else _p(mo, _u32p), None if rng[0] is None else _p(rng[0], _u32p),
            None if rng[1] is None else _p(rng[1], _u32p), _p(ids, _u32p), _p(dists, _f32p), _p(labels, _u32p),
            _p(sizes, _u32p), _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, labels, sizes, counts, stats.view(np.uint32).astype(np.int64)

    def group_by_label_device(self, nq, pool, n_groups, per_group, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids,
                              d_dists, d_group_labels, d_group_sizes, d_counts=None, d_stats=None, stream=0):
        """hnsw_group_by_label_device over torch device tensors (or raw device pointers): the [nq, pool] candidate lists
        a *_device search of this index left (d_counts_in / d_stats_in [nq] or None), collapsed by this index's labels
        into d_ids / d_dists [nq, n_groups, per_group], d_group_labels / d_group_sizes [nq, n_groups] (/ d_counts /
        d_stats).  ONE launch enqueued on `stream`, no sync of it."""
        p = self._dptr
        check(self._L.hnsw_group_by_label_device(
            self._h, nq, pool, n_groups, per_group, p(d_ids_in), p(d_dists_in), p(d_counts_in), p(d_stats_in), p(d_ids),
            p(d_dists), p(d_group_labels), p(d_group_sizes), p(d_counts), p(d_stats), stream or None))

    # ---- radius search: every neighbour within a distance (include/hnsw_mi355x.h) ----------------------------------
    def search_batch_radius(self, Q, radius, n_first=16, max_n=256, ef=0):
        """Every neighbour of a query within its radius, out of the candidate lists that search_batch returns on a
        ladder of n = n_first, 2 n_first, ... up to max_n with ef = max(ef, n) (hnsw_search_batch_radius).  radius:
        [nq], or a scalar broadcast to all queries; in the unit of the returned distances, >= 0, +inf is legal.
        -> ids [nq, max_n] (pad UINT32_MAX), dists [nq, max_n] (pad +inf), counts [nq], flags [nq] (RADIUS_MORE:
        truncated at max_n), rungs [nq] (searches the query took part in), stats [nq, 4] (its last rung's)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq, width = Q.shape[0], max(int(max_n), 1)
        radius = np.asarray(radius, dtype=np.float32)
        if radius.ndim > 1 or (radius.ndim == 1 and radius.shape[0] != nq):
            raise ValueError("radius is a scalar or one value per query")
        radius = np.ascontiguousarray(np.broadcast_to(radius, (nq,)))
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, width), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        flags = np.zeros(nq, dtype=np.uint32)
        rungs = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_radius(
            self._h, _p(Q, _f32p), nq, _p(radius, _f32p), n_first, max_n, ef, _p(ids, _u32p), _p(dists, _f32p),
            _p(counts, _u32p), _p(flags, _u32p), _p(rungs, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, counts, flags, rungs, stats.view(np.uint32).astype(np.int64)

    @staticmethod
    def radius_cut_device(nq, n_in, n_out, d_radius, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
                          d_counts=None, d_flags=None, d_stats=None, d_sel=None, n_sel=0, stream=0):
        """hnsw_radius_cut_device over torch device tensors (or raw device pointers): the [nq, n_in] candidate lists a
        *_device search left (d_counts_in / d_stats_in [nq] or None), cut at d_radius [nq] into d_ids / d_dists
        [nq, n_out] (/ d_counts / d_flags / d_stats), for the n_sel queries of d_sel or, with d_sel None, for all.
        ONE launch enqueued on `stream` of the current device, no sync of it; needs no index."""
        p = HNSW._dptr
        check(_lib.lib().hnsw_radius_cut_device(
            nq, n_in, n_out, p(d_radius), p(d_sel), n_sel, p(d_ids_in), p(d_dists_in), p(d_counts_in), p(d_stats_in),
            p(d_ids), p(d_dists), p(d_counts), p(d_flags), p(d_stats), stream or None))

    # ---- diversified search: maximal marginal relevance (include/hnsw_mi355x.h) ------------------------------------
    def search_batch_diverse(self, Q, n, pool, ef, lam=0.5, mask_set=None, mask_of=None, lo=None, hi=None):
        """n hits per query that are near the query and not near each other: the MMR selection (diverse.mmr_select,
        lambda = lam in [0, 1]) out of the `pool` candidates that search_batch (or, with mask_set / lo and hi, the
        filtered search of that kind) returns with n = pool (hnsw_search_batch_diverse).  mask_of [nq]: rows of the
        set, -1 or MASK_NONE; None: row 0.  lo / hi: both or neither, scalars broadcast.
        -> ids [nq, n] (pad UINT32_MAX), dists [nq, n] (pad +inf), gaps [nq, n] (a hit's distance to the nearest hit
        before it; +inf for the first and the pad), counts [nq], stats [nq, 4] (the candidate call's), all in
        selection order"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        if (lo is None) != (hi is None):
            raise ValueError("a label range needs lo and hi, both or neither")
        nq, width = Q.shape[0], max(int(n), 1)
        mo = self._mask_of(mask_of, nq)
        rng = (None, None) if lo is None else self._range(lo, hi, nq)
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, width), np.inf, dtype=np.float32)
        gaps = np.full((nq, width), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_diverse(
            self._h, _p(Q, _f32p), nq, n, pool, ef, float(lam), mask_set._s if mask_set is not None else None,
            None if mo is None else _p(mo, _u32p), None if rng[0] is None else _p(rng[0], _u32p),
            None if rng[1] is None else _p(rng[1], _u32p), _p(ids, _u32p), _p(dists, _f32p), _p(gaps, _f32p),
            _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, gaps, counts, stats.view(np.uint32).astype(np.int64)

    def diversify_device(self, nq, pool, n_out, lam, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
                         d_gaps=None, d_counts=None, d_stats=None, stream=0):
        """hnsw_diversify_device over torch device tensors (or raw device pointers): the [nq, pool] candidate lists a
        *_device search of this index left (d_counts_in / d_stats_in [nq] or None), re-ranked by MMR over this index's
        stored rows into d_ids / d_dists [nq, n_out] (/ d_gaps / d_counts / d_stats).  ONE launch enqueued on `stream`,
        no sync of it."""
        p = self._dptr
        check(self._L.hnsw_diversify_device(
            self._h, nq, pool, n_out, float(lam), p(d_ids_in), p(d_dists_in), p(d_counts_in), p(d_stats_in), p(d_ids),
            p(d_dists), p(d_gaps), p(d_counts), p(d_stats), stream or None))

    # ---- search from stored rows: queries by id and by weighted ids (include/hnsw_mi355x.h) ------------------------
    def search_batch_from_rows(self, src_ids, weights, n, ef, exclude=True):
        """The n nearest of queries composed out of stored rows (from_rows.compose_rows): src_ids [nq, width] (a slot
        holding UINT32_MAX is absent), weights [nq, width] float32 or None (every weight 1.0).  exclude: the sources
        are taken out of their own lists (from_rows.drop_ids over the search with n + width); False: they stay, and the
        call is search_batch of the composed rows (hnsw_search_batch_from_rows).
        -> ids [nq, n] (pad UINT32_MAX), dists [nq, n] (pad +inf), counts [nq], stats [nq, 4]"""
        src = np.ascontiguousarray(src_ids, dtype=np.uint32)
        if src.ndim != 2:
            raise ValueError("src_ids is [nq, width]")
        nq, width = src.shape
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != src.shape:
                raise ValueError("weights has the shape of src_ids")
        ids = np.full((nq, max(int(n), 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(int(n), 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_from_rows(
            self._h, _p(src, _u32p), None if w is None else _p(w, _f32p), nq, width, n, ef, 1 if exclude else 0,
            _p(ids, _u32p), _p(dists, _f32p), _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, counts, stats.view(np.uint32).astype(np.int64)

    def search_batch_by_id(self, src_ids, n, ef, exclude_self=True):
        """The n nearest of the stored rows src_ids [nq], each without itself unless exclude_self is False
        (hnsw_search_batch_by_id: search_batch_from_rows with one slot and no weights).
        -> ids [nq, n] (pad UINT32_MAX), dists [nq, n] (pad +inf), counts [nq], stats [nq, 4]"""
        src = np.ascontiguousarray(src_ids, dtype=np.uint32).reshape(-1)
        nq = src.shape[0]
        ids = np.full((nq, max(int(n), 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(int(n), 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_by_id(
            self._h, _p(src, _u32p), nq, n, ef, 1 if exclude_self else 0, _p(ids, _u32p), _p(dists, _f32p),
            _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, counts, stats.view(np.uint32).astype(np.int64)

    def knn_graph(self, n, ef, chunk=65536, ids=None, exclude_self=True):
        """The k-NN graph of the index: search_batch_by_id over all ids (or the given ones), `chunk` sources a call.
        -> ids [N, n] (pad UINT32_MAX), dists [N, n] (pad +inf), counts [N]"""
        src = np.arange(self.len(), dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        chunk = max(int(chunk), 1)
        o_ids = np.full((src.shape[0], max(int(n), 1)), _lib.UINT32_MAX, dtype=np.uint32)
        o_dists = np.full((src.shape[0], max(int(n), 1)), np.inf, dtype=np.float32)
        o_counts = np.zeros(src.shape[0], dtype=np.uint32)
        for a in range(0, src.shape[0], chunk):
            b = min(a + chunk, src.shape[0])
            o_ids[a:b], o_dists[a:b], o_counts[a:b], _ = self.search_batch_by_id(src[a:b], n, ef, exclude_self)
        return o_ids, o_dists, o_counts

    def compose_rows_device(self, nq, width, d_src_ids, d_weights, d_Q, d_status=None, stream=0):
        """hnsw_compose_rows_device over torch device tensors (or raw device pointers): d_src_ids uint32 [nq, width],
        d_weights float32 [nq, width] or None, composed out of this index's stored rows into d_Q float32 [nq, dim]
        (/ d_status int32 [nq]).  ONE launch enqueued on `stream`, no sync of it."""
        p = self._dptr
        check(self._L.hnsw_compose_rows_device(self._h, nq, width, p(d_src_ids), p(d_weights), p(d_Q), p(d_status),
                                               stream or None))

    @staticmethod
    def drop_ids_device(nq, n_in, n_out, width, d_ex, d_src_status, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids,
                        d_dists, d_counts=None, d_dropped=None, d_stats=None, stream=0):
        """hnsw_drop_ids_device over torch device tensors (or raw device pointers): the [nq, n_in] candidate lists a
        *_device search left (d_counts_in / d_stats_in [nq] or None) without the ids of d_ex uint32 [nq, width]
        (d_src_status int32 [nq] or None: the compose statuses), into d_ids / d_dists [nq, n_out] (/ d_counts /
        d_dropped / d_stats).  ONE launch enqueued on `stream` of the current device, no sync of it; needs no index."""
        p = HNSW._dptr
        check(_lib.lib().hnsw_drop_ids_device(
            nq, n_in, n_out, width, p(d_ex), p(d_src_status), p(d_ids_in), p(d_dists_in), p(d_counts_in), p(d_stats_in),
            p(d_ids), p(d_dists), p(d_counts), p(d_dropped), p(d_stats), stream or None))

    # ---- multi-vector search: several vectors per query, their lists fused (include/hnsw_mi355x.h) -----------------
    def search_batch_multi(self, Q, n, pool, ef, weights=None, mode="sum"):
        """The n best of queries of T vectors each, Q [nq, T, dim]: every vector is searched with n = pool, and the
        distinct ids of a query's T lists are scored against all T vectors -- mode "sum": the sum of weights[q, t] *
        distance, "min": the smallest of them -- and ranked by (score, id): multi.fuse_lists over search_batch of the
        nq * T rows (hnsw_search_batch_multi).  weights [nq, T] float32 or None (no multiply).  The answer is the best n
        of the UNION of the per-vector pools, not of the whole index.
        -> ids [nq, n] (pad UINT32_MAX), scores [nq, n] (pad +inf), counts [nq], unique [nq] (distinct candidates),
        stats [nq, 4] (the summed counters of the T searches)"""
        from .multi import mode_of
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 3 or Q.shape[2] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x T x %d" % self.dim)
        nq, T = Q.shape[0], Q.shape[1]
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != (nq, T):
                raise ValueError("weights is [nq, T]")
        width = max(int(n), 1)
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        scores = np.full((nq, width), np.inf, dtype=np.float32)
        counts, unique = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_multi(
            self._h, _p(Q, _f32p), nq, T, None if w is None else _p(w, _f32p), mode_of(mode), n, pool, ef, _p(ids, _u32p),
            _p(scores, _f32p), _p(counts, _u32p), _p(unique, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, scores, counts, unique, stats.view(np.uint32).astype(np.int64)

    def fuse_lists_device(self, nq, n_vecs, pool, n_out, mode, d_Q, d_weights, d_ids_in, d_counts_in, d_stats_in, d_ids,
                          d_scores, d_counts=None, d_unique=None, d_stats=None, stream=0):
        """hnsw_fuse_lists_device over torch device tensors (or raw device pointers): d_Q float32 [nq, n_vecs, dim],
        d_weights float32 [nq, n_vecs] or None, and the [nq, n_vecs, pool] candidate ids a *_device search of this index
        left for the nq * n_vecs rows of d_Q (d_counts_in / d_stats_in [nq, n_vecs] or None), fused over this index's
        stored rows into d_ids / d_scores [nq, n_out] (/ d_counts / d_unique / d_stats).  ONE launch enqueued on
        `stream`, no sync of it."""
        from .multi import mode_of
        p = self._dptr
        check(self._L.hnsw_fuse_lists_device(
            self._h, nq, n_vecs, pool, n_out, mode_of(mode), p(d_Q), p(d_weights), p(d_ids_in), p(d_counts_in), p(d_stats_in),
            p(d_ids), p(d_scores), p(d_counts), p(d_unique), p(d_stats), stream or None))

    # ---- hybrid search: rank fusion of the index's hits with external ranked lists (include/hnsw_mi355x.h) -----------
    @staticmethod
    def _hybrid_weights(weights, nq, E):
        """None, [1 + E] (broadcast over the queries) or [nq, 1 + E] -> float32 [nq, 1 + E] or None"""
        if weights is None:
            return None
        w = np.asarray(weights, dtype=np.float32)
        if w.shape == (1 + E,):
            w = np.broadcast_to(w, (nq, 1 + E))
        if w.shape != (nq, 1 + E):
            raise ValueError("weights is [1 + E] or [nq, 1 + E]: slot 0 is the dense slot")
        return np.ascontiguousarray(w, dtype=np.float32)

    def search_batch_hybrid(self, Q, n, pool, ef, ext_ids=None, ext_scores=None, ext_counts=None, mode="rrf", rank_constant=60,
                            weights=None, absent=None, mask_set=None, mask_of=None, lo=None, hi=None):
        """The n best of the index's own `pool` hits fused with E external ranked lists per query -- BM25, a sparse model,
        another index -- by reciprocal rank ("rrf": larger is better) or by a weighted sum of the dense distance and the
        external scores ("linear": smaller is better), every list under this index's deletions and, with mask_set / lo
        and hi, its mask rows and label range: hybrid.fuse_ranked over search_batch (or the filtered search of that
        kind) with n = pool (hnsw_search_batch_hybrid).  ext_ids [nq, E, W] uint32 (pad UINT32_MAX) or None, ext_scores
        [nq, E, W] float32 (required under "linear" with E > 0), ext_counts [nq, E] or None, weights [1 + E] or
        [nq, 1 + E] or None, absent [E] or None.
        -> ids [nq, n] (pad UINT32_MAX), scores [nq, n] (pad -inf / +inf), dists [nq, n] (each hit's own distance, pad
        +inf), counts [nq], unique [nq], dropped [nq] (entries the filter removed), stats [nq, 4] (the dense call's)"""
        from .hybrid import mode_of
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        if (lo is None) != (hi is None):
            raise ValueError("a label range needs lo and hi, both or neither")
        nq, width = Q.shape[0], max(int(n), 1)
        E, W, e_ids, e_sc, e_cnt = 0, 0, None, None, None
        if ext_ids is not None:
            e_ids = np.ascontiguousarray(ext_ids, dtype=np.uint32)
            if e_ids.ndim != 3 or e_ids.shape[0] != nq:
                raise ValueError("ext_ids is [nq, E, ext_width]")
            E, W = e_ids.shape[1], e_ids.shape[2]
            if ext_scores is not None:
                e_sc = np.ascontiguousarray(ext_scores, dtype=np.float32)
                if e_sc.shape != e_ids.shape:
                    raise ValueError("ext_scores has the shape of ext_ids")
            if ext_counts is not None:
                e_cnt = np.ascontiguousarray(ext_counts, dtype=np.uint32).reshape(nq, E)
        w = self._hybrid_weights(weights, nq, E)
        ab = None if absent is None else np.ascontiguousarray(absent, dtype=np.float32).reshape(E)
        mo = self._mask_of(mask_of, nq)
        rng = (None, None) if lo is None else self._range(lo, hi, nq)
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        scores = np.zeros((nq, width), dtype=np.float32)
        dists = np.full((nq, width), np.inf, dtype=np.float32)
        counts, unique, dropped = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
        stats = np.zeros((nq, 4), dtype=np.int32)
        opt = lambda a, t: None if a is None else _p(a, t)  # noqa: E731
        check(self._L.hnsw_search_batch_hybrid(
            self._h, _p(Q, _f32p), nq, n, pool, ef, mode_of(mode), rank_constant, E, W, opt(e_ids, _u32p), opt(e_sc, _f32p),
            opt(e_cnt, _u32p), opt(w, _f32p), opt(ab, _f32p), mask_set._s if mask_set is not None else None, opt(mo, _u32p),
            opt(rng[0], _u32p), opt(rng[1], _u32p), _p(ids, _u32p), _p(scores, _f32p), _p(dists, _f32p), _p(counts, _u32p),
            _p(unique, _u32p), _p(dropped, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, scores, dists, counts, unique, dropped, stats.view(np.uint32).astype(np.int64)

    def fuse_ranked_device(self, nq, mode, rank_constant, n_out, pool, d_ids0, d_counts0, d_stats0, n_ext, ext_width, d_ext_ids,
                           d_ext_scores, d_ext_counts, d_weights, absent, d_Q, d_ids, d_scores, d_dists=None, d_counts=None,
                           d_unique=None, d_dropped=None, d_stats=None, mask_set=None, d_mask_of=None, d_lo=None, d_hi=None,
                           stream=0):
        """hnsw_fuse_ranked_device over torch device tensors (or raw device pointers): the dense list d_ids0 [nq, pool]
        (/ d_counts0 / d_stats0 [nq]; None: no dense list) a *_device search of this index left, fused with the n_ext
        external lists d_ext_ids / d_ext_scores [nq, n_ext, ext_width] (/ d_ext_counts [nq, n_ext]) under d_weights
        [nq, 1 + n_ext] (or None), `absent` (HOST: [n_ext] floats or None), optionally d_Q float32 [nq, dim], and the
        filter (mask_set, d_mask_of / d_lo / d_hi [nq]), into d_ids / d_scores [nq, n_out] (/ d_dists / d_counts /
        d_unique / d_dropped / d_stats).  ONE launch enqueued on `stream`, no sync of it."""
        from .hybrid import mode_of
        p = self._dptr
        ab = None if absent is None else np.ascontiguousarray(absent, dtype=np.float32).reshape(n_ext)
        check(self._L.hnsw_fuse_ranked_device(
            self._h, nq, mode_of(mode), rank_constant, n_out, pool, p(d_ids0), p(d_counts0), p(d_stats0), n_ext, ext_width,
            p(d_ext_ids), p(d_ext_scores), p(d_ext_counts), p(d_weights), None if ab is None else _p(ab, _f32p), p(d_Q),
            mask_set._s if mask_set is not None else None, p(d_mask_of), p(d_lo), p(d_hi), p(d_ids), p(d_scores), p(d_dists),
            p(d_counts), p(d_unique), p(d_dropped), p(d_stats), stream or None))

    # ---- late-interaction search: documents of several rows scored by summed min distance (include/hnsw_mi355x.h) ----
    def search_batch_late(self, Q, n, pool, ef, mode="sum"):
        """The n best DOCUMENTS -- the rows that share a label (set_labels) -- of queries of T vectors each, Q [nq, T, dim]:
        every vector is searched with n = pool, and a document with a row among the distinct ids of a query's T lists is
        scored by the sum over the vectors of the distance (mode "sum"; "sum_sq": its square, MaxSim's ranking on
        unit-length rows) to its nearest row among them: late.late_interaction over search_batch of the nq * T rows
        (hnsw_search_batch_late).  A document's minimum runs over its rows in the pools, not over all its stored rows.
        -> doc_labels [nq, n] (pad 0), scores [nq, n] (pad +inf), best_ids [nq, n] (pad UINT32_MAX: the row to show as
        the hit), doc_sizes [nq, n] (pad 0), counts [nq], n_docs [nq], stats [nq, 4] (the summed counters of the T
        searches)"""
        from .late import mode_of
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 3 or Q.shape[2] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x T x %d" % self.dim)
        nq, T = Q.shape[0], Q.shape[1]
        width = max(int(n), 1)
        labels = np.zeros((nq, width), dtype=np.uint32)
        scores = np.full((nq, width), np.inf, dtype=np.float32)
        best = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        sizes = np.zeros((nq, width), dtype=np.uint32)
        counts, n_docs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_late(
            self._h, _p(Q, _f32p), nq, T, mode_of(mode), n, pool, ef, _p(labels, _u32p), _p(scores, _f32p), _p(best, _u32p),
            _p(sizes, _u32p), _p(counts, _u32p), _p(n_docs, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return labels, scores, best, sizes, counts, n_docs, stats.view(np.uint32).astype(np.int64)

    def late_interaction_device(self, nq, n_vecs, pool, n_out, mode, d_Q, d_ids_in, d_counts_in, d_stats_in, d_doc_labels,
                                d_scores, d_best_ids=None, d_doc_sizes=None, d_counts=None, d_n_docs=None, d_stats=None,
                                stream=0):
        """hnsw_late_interaction_device over torch device tensors (or raw device pointers): d_Q float32 [nq, n_vecs, dim]
        and the [nq, n_vecs, pool] candidate ids a *_device search of this index left for the nq * n_vecs rows of d_Q
        (d_counts_in / d_stats_in [nq, n_vecs] or None), scored as documents over this index's stored rows and labels
        into d_doc_labels / d_scores [nq, n_out] (/ d_best_ids / d_doc_sizes / d_counts / d_n_docs / d_stats).  ONE launch
        enqueued on `stream`, no sync of it."""
        from .late import mode_of
        p = self._dptr
        check(self._L.hnsw_late_interaction_device(
            self._h, nq, n_vecs, pool, n_out, mode_of(mode), p(d_Q), p(d_ids_in), p(d_counts_in), p(d_stats_in),
            p(d_doc_labels), p(d_scores), p(d_best_ids), p(d_doc_sizes), p(d_counts), p(d_n_docs), p(d_stats), stream or None))

    # ---- exact document scoring: late interaction over every stored row (include/hnsw_mi355x.h) ----------------------
    def search_batch_late_exact(self, Q, n, n_cand, pool, ef, mode="sum", rows_cap=_lib.DOCS_MAX_ROWS):
        """search_batch_late with every returned document scored over ALL its undeleted rows: the n_cand best documents
        of the late interaction over the pools are scored again over their min(size, rows_cap) lowest ids, and the n best
        of them returned: docs.score_documents of late.late_interaction's labels (hnsw_search_batch_late_exact).
        -> doc_labels [nq, n] (pad 0), scores [nq, n] (pad +inf), best_ids [nq, n] (pad UINT32_MAX), doc_sizes [nq, n]
        (pad 0: the full size), counts [nq], n_docs [nq], stats [nq, 4] (the summed counters of the T searches)"""
        from .late import mode_of
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 3 or Q.shape[2] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x T x %d" % self.dim)
        nq, T = Q.shape[0], Q.shape[1]
        width = max(int(n), 1)
        labels = np.zeros((nq, width), dtype=np.uint32)
        scores = np.full((nq, width), np.inf, dtype=np.float32)
        best = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        sizes = np.zeros((nq, width), dtype=np.uint32)
        counts, n_docs = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_late_exact(
            self._h, _p(Q, _f32p), nq, T, mode_of(mode), n, n_cand, rows_cap, pool, ef, _p(labels, _u32p), _p(scores, _f32p),
            _p(best, _u32p), _p(sizes, _u32p), _p(counts, _u32p), _p(n_docs, _u32p),
            C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return labels, scores, best, sizes, counts, n_docs, stats.view(np.uint32).astype(np.int64)

    def score_documents_device(self, nq, n_vecs, n_in, n_out, rows_cap, mode, d_Q, d_docs_in, d_counts_in, d_stats_in,
                               d_doc_labels, d_scores, d_best_ids=None, d_doc_sizes=None, d_counts=None, d_n_docs=None,
                               d_stats=None, stream=0):
        """hnsw_score_documents_device over torch device tensors (or raw device pointers): d_Q float32 [nq, n_vecs, dim]
        and the [nq, n_in] document LABELS (d_counts_in / d_stats_in [nq] or None), every document scored over its
        min(size, rows_cap) lowest undeleted ids into d_doc_labels / d_scores [nq, n_out] (/ d_best_ids / d_doc_sizes /
        d_counts / d_n_docs / d_stats).  ONE launch enqueued on `stream`, no sync of it."""
        from .late import mode_of
        p = self._dptr
        check(self._L.hnsw_score_documents_device(
            self._h, nq, n_vecs, n_in, n_out, rows_cap, mode_of(mode), p(d_Q), p(d_docs_in), p(d_counts_in), p(d_stats_in),
            p(d_doc_labels), p(d_scores), p(d_best_ids), p(d_doc_sizes), p(d_counts), p(d_n_docs), p(d_stats), stream or None))

    # ---- refined search: the pool re-scored against full rows kept in HBM (include/hnsw_mi355x.h) -------------------
    def row_table(self, full_dim, dtype="f32"):
        """-> refine.RowTable: full rows of full_dim elements, "f32" or "f16", that live in HBM beside this index, row id =
        index id (hnsw_row_table).  Making one needs no GPU; the first write allocates."""
        from .refine import RowTable, dtype_of
        t = C.c_void_p()
        check(self._L.hnsw_row_table_create(self._h, int(full_dim), dtype_of(dtype), C.byref(t)))
        return RowTable(self, t)

    def search_batch_refined(self, table, Q, Qfull, n, pool, ef, mask_set=None, mask_of=None, lo=None, hi=None):
        """The n nearest by the FULL rows of `table` (a RowTable of this index) out of the `pool` candidates that
        search_batch (or, with mask_set / lo and hi, the filtered search of that kind) returns for Q with n = pool:
        refine.refine_lists of those lists with Qfull [nq, full_dim] (hnsw_search_batch_refined).  Q None: the index's
        queries are the first dim elements of each Qfull row.  The cosine option applies to Q alone.
        -> ids [nq, n] (pad UINT32_MAX), dists [nq, n] (the full rows' distances, pad +inf), counts [nq], stats [nq, 4]
        (the candidate call's)"""
        Qfull = np.ascontiguousarray(Qfull, dtype=np.float32)
        if Qfull.ndim != 2 or Qfull.shape[1] != table.full_dim:
            raise HnswError(_lib.ERR_BAD_DIM, "full queries must be nq x %d" % table.full_dim)
        nq, width = Qfull.shape[0], max(int(n), 1)
        if Q is not None:
            Q = np.ascontiguousarray(Q, dtype=np.float32)
            if Q.ndim != 2 or Q.shape[1] != self.dim or Q.shape[0] != nq:
                raise HnswError(_lib.ERR_BAD_DIM, "queries must be %d x %d" % (nq, self.dim))
        if (lo is None) != (hi is None):
            raise ValueError("a label range needs lo and hi, both or neither")
        mo = self._mask_of(mask_of, nq)
        rng = (None, None) if lo is None else self._range(lo, hi, nq)
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, width), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_refined(
            self._h, table._t, None if Q is None else _p(Q, _f32p), _p(Qfull, _f32p), nq, n, pool, ef,
            mask_set._s if mask_set is not None else None, None if mo is None else _p(mo, _u32p),
            None if rng[0] is None else _p(rng[0], _u32p), None if rng[1] is None else _p(rng[1], _u32p), _p(ids, _u32p),
            _p(dists, _f32p), _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, dists, counts, stats.view(np.uint32).astype(np.int64)

    @staticmethod
    def refine_device(nq, pool, n_out, full_dim, dtype, d_table, table_rows, d_Qfull, d_ids_in, d_counts_in, d_stats_in,
                      d_ids, d_dists, d_counts=None, d_stats=None, stream=0):
        """hnsw_refine_device over torch device tensors (or raw device pointers): refine.refine_device.  ONE launch
        enqueued on `stream` of the current device, no sync of it; needs no index."""
        from .refine import refine_device
        refine_device(nq, pool, n_out, full_dim, dtype, d_table, table_rows, d_Qfull, d_ids_in, d_counts_in, d_stats_in,
                      d_ids, d_dists, d_counts, d_stats, stream)

    # ---- boosted search: the pool re-ranked by per-id attributes kept in HBM (include/hnsw_mi355x.h) ----------------
    def search_batch_boosted(self, table, Q, weights, n, pool, ef, mask_set=None, mask_of=None, lo=None, hi=None):
        """The n best by w[0] * distance + sum_k w[1 + k] * attribute k (SMALLER is better) out of the `pool` candidates
        that search_batch (or, with mask_set / lo and hi, the filtered search of that kind) returns for Q with n = pool:
        boost.boost_lists of those lists over `table` (a RowTable of this index with at most 32 columns) under weights
        [1 + A] (one row for every query) or [nq, 1 + A] (hnsw_search_batch_boosted).
        -> ids [nq, n] (pad UINT32_MAX), scores [nq, n] (pad +inf), dists [nq, n] (the hits' own distances, pad +inf),
        counts [nq], stats [nq, 4] (the candidate call's)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq, width = Q.shape[0], max(int(n), 1)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.ndim == 1:
            weights = weights.reshape(1, -1)
        if weights.ndim != 2 or weights.shape[1] != 1 + table.full_dim:
            raise HnswError(_lib.ERR_BAD_DIM, "weights must be [1 + %d] or nq x (1 + %d)" % (table.full_dim, table.full_dim))
        if (lo is None) != (hi is None):
            raise ValueError("a label range needs lo and hi, both or neither")
        mo = self._mask_of(mask_of, nq)
        rng = (None, None) if lo is None else self._range(lo, hi, nq)
        ids = np.full((nq, width), _lib.UINT32_MAX, dtype=np.uint32)
        scores = np.full((nq, width), np.inf, dtype=np.float32)
        dists = np.full((nq, width), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        check(self._L.hnsw_search_batch_boosted(
            self._h, table._t, _p(Q, _f32p), nq, n, pool, ef, _p(weights, _f32p), weights.shape[0],
            mask_set._s if mask_set is not None else None, None if mo is None else _p(mo, _u32p),
            None if rng[0] is None else _p(rng[0], _u32p), None if rng[1] is None else _p(rng[1], _u32p), _p(ids, _u32p),
            _p(scores, _f32p), _p(dists, _f32p), _p(counts, _u32p), C.cast(stats.ctypes.data, C.POINTER(QueryStats))))
        return ids, scores, dists, counts, stats.view(np.uint32).astype(np.int64)

    @staticmethod
    def boost_device(nq, pool, n_out, n_attrs, dtype, d_table, table_rows, d_weights, weights_rows, d_ids_in, d_dists_in,
                     d_counts_in, d_stats_in, d_ids, d_scores, d_dists=None, d_counts=None, d_stats=None, stream=0):
        """hnsw_boost_device over torch device tensors (or raw device pointers): boost.boost_device.  ONE launch enqueued
        on `stream` of the current device, no sync of it; needs no index."""
        from .boost import boost_device
        boost_device(nq, pool, n_out, n_attrs, dtype, d_table, table_rows, d_weights, weights_rows, d_ids_in, d_dists_in,
                     d_counts_in, d_stats_in, d_ids, d_scores, d_dists, d_counts, d_stats, stream)

    def load_row_table(self, path):
        """-> refine.RowTable: the table RowTable.save wrote to `path`, created on this index and written to its device
        (hnsw_row_table_load).  A file that is not a whole, finite row table raises (ERR_IO) before any device is touched,
        but for a NaN or an infinity among its elements."""
        from .refine import RowTable
        t = C.c_void_p()
        check(self._L.hnsw_row_table_load(self._h, str(path).encode(), C.byref(t)))
        return RowTable(self, t)

    def search_filtered(self, q, n, ef, lo=0, hi=0xFFFFFFFF, mask_set=None, row=None):
        """ONE query under the label range [lo, hi] and, with a resident MaskSet, its row `row` (None, -1 or MASK_NONE: no
        row): hnsw_search_filtered, whose concurrent callers on an index are gathered into one launch.
        -> (ids [n], dists [n], count, path)"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
        if q.shape[0] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "the query must have %d values" % self.dim)
        row = _lib.MASK_NONE if row is None or int(row) < 0 else int(row)
        ids = np.full(max(n, 1), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full(max(n, 1), np.inf, dtype=np.float32)
        count, path = C.c_uint32(), C.c_uint8()
        check(self._L.hnsw_search_filtered(self._h, _p(q, _f32p), n, ef, mask_set._s if mask_set is not None else None, row,
                                           int(lo), int(hi), _p(ids, _u32p), _p(dists, _f32p), C.byref(count), C.byref(path)))
        return ids[:n], dists[:n], count.value, path.value

    def search_filtered_threads(self, Q, n, ef, lo, hi, threads, seconds, mask_set=None, row=None):
        """hnsw_bench_search_filtered_threads: `threads` host threads, each blocked in its own hnsw_search_filtered call;
        query i under row[i] of mask_set (both None: no set; -1 or MASK_NONE: no row) and [lo[i], hi[i]] (scalars
        broadcast).  -> (ids [nq, n], dists, counts, paths, rcs [nq]: every query's last answer and status, calls, wall
        seconds, the latency dict of search_threads)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq = Q.shape[0]
        lo, hi = self._range(lo, hi, nq)
        rows = None
        if mask_set is not None:
            rows = np.broadcast_to(np.asarray(-1 if row is None else row, dtype=np.int64), (nq,))
            rows = np.ascontiguousarray(np.where(rows < 0, _lib.MASK_NONE, rows).astype(np.uint32))
        ids = np.full((nq, max(n, 1)), _lib.UINT32_MAX, dtype=np.uint32)
        dists = np.full((nq, max(n, 1)), np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        paths = np.zeros(nq, dtype=np.uint8)
        rcs = np.zeros(nq, dtype=np.int32)
        calls, wall = C.c_uint64(), C.c_double()
        lat = (C.c_double * 7)()
        check(self._L.hnsw_bench_search_filtered_threads(
            self._h, _p(Q, _f32p), nq, n, ef, mask_set._s if mask_set is not None else None,
            _p(rows, _u32p) if rows is not None else None, _p(lo, _u32p), _p(hi, _u32p), int(threads), float(seconds),
            _p(ids, _u32p), _p(dists, _f32p), _p(counts, _u32p), _p(paths, _lib.u8p), rcs.ctypes.data_as(C.POINTER(C.c_int32)),
            C.byref(calls), C.byref(wall), lat))
        return (ids[:, :n], dists[:, :n], counts, paths, rcs, calls.value, wall.value,
                dict(zip(("p50", "p90", "p99", "max", "mean", "cpu_user_s", "cpu_sys_s"), list(lat))))

    def ann_by_vector_filtered(self, vector, n, ef, allow):
        """ann_by_vector restricted to the allowed ids -> list of ids"""
        q = np.ascontiguousarray(vector, dtype=np.float32).reshape(1, -1)
        ids, _, counts, _, _ = self.search_batch_filtered(q, n, ef, allow)
        return [int(x) for x in ids[0, : counts[0]]]

    def search_batch_device(self, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats, stream=0):
        """All arguments are raw device pointers (ints); enqueues on `stream`, no sync."""
        check(self._L.hnsw_search_batch_device(self._h, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats,
                                               stream))

    def search_batch_device_finish(self, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats, stream=0):
        """Completes search_batch_device: synchronises, re-runs queries whose visited table overflowed,
        raises the first per-query error."""
        check(self._L.hnsw_search_batch_device_finish(self._h, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats,
                                                      stream))

    def distance_batch(self, q, ids):
        """VecBase::dist2many seam on the device"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(ids.shape[0], dtype=np.float32)
        check(self._L.hnsw_distance_batch(self._h, _p(q, _f32p), _p(ids, _u32p), ids.shape[0],
                                          _p(out, _f32p)))
        return out

    def search_layer(self, layer, q, entry_ids, ef):
        """Searcher::search_layer seam on the device -> (ids, dists, stats)"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
        e = np.ascontiguousarray(entry_ids, dtype=np.uint32)
        ids = np.zeros(max(ef, 1), dtype=np.uint32)
        dists = np.zeros(max(ef, 1), dtype=np.float32)
        cnt = C.c_uint32()
        st = QueryStats()
        check(self._L.hnsw_search_layer(self._h, layer, _p(q, _f32p), _p(e, _u32p), e.shape[0], ef,
                                        _p(ids, _u32p), _p(dists, _f32p), C.byref(cnt), C.byref(st)))
        return ids[: cnt.value].copy(), dists[: cnt.value].copy(), (st.n_dist, st.n_exp, st.sum_deg)

    def brute_force(self, Q, k):
        """exact top-k under the index's own metric, on the device"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq = Q.shape[0]
        ids = np.zeros((nq, k), dtype=np.uint32)
        dists = np.zeros((nq, k), dtype=np.float32)
        check(self._L.hnsw_brute_force(self._h, _p(Q, _f32p), nq, k, _p(ids, _u32p), _p(dists, _f32p)))
        return ids, dists

    def brute_force_fast(self, Q, k):
        """ground truth on the matrix cores (MFMA screen + exact re-rank of the k + 8 best): f32 rows only;
        not bit-exact by construction, see include/hnsw_mi355x.h"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq = Q.shape[0]
        ids = np.zeros((nq, k), dtype=np.uint32)
        dists = np.zeros((nq, k), dtype=np.float32)
        check(self._L.hnsw_brute_force_fast(self._h, _p(Q, _f32p), nq, k, _p(ids, _u32p), _p(dists, _f32p)))
        return ids, dists

    # ---- deletion (include/hnsw_mi355x.h: deleted ids stay in the graph, no search returns them) ---------------
    def _ids(self, ids):
        a = np.asarray(ids).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > _lib.UINT32_MAX):
            raise HnswError(_lib.ERR_ARG, "ids must be in [0, 2^32)")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def mark_deleted(self, ids):
        """hnswlib's mark_deleted for an id or an array of ids; every id must be < len (else nothing changes)"""
        a = self._ids(ids)
        check(self._L.hnsw_mark_deleted(self._h, _p(a, _u32p), a.shape[0]))

    def unmark_deleted(self, ids):
        a = self._ids(ids)
        check(self._L.hnsw_unmark_deleted(self._h, _p(a, _u32p), a.shape[0]))

    def is_deleted(self, node):
        out = C.c_int()
        check(self._L.hnsw_is_deleted(self._h, int(node), C.byref(out)))
        return bool(out.value)

    def deleted_count(self):
        return int(self._L.hnsw_deleted_count(self._h))

    def deleted_ids(self):
        """-> the deleted ids, ascending (uint32)"""
        n = C.c_uint64()
        check(self._L.hnsw_get_deleted(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        check(self._L.hnsw_get_deleted(self._h, _p(out, _u32p), out.shape[0], C.byref(n)))
        return out

    # ---- accessors ------------------------------------------------------------------------------
    def len(self):
        return int(self._L.hnsw_len(self._h))

    def __len__(self):
        return self.len()

    def distance(self, a, b):
        """HNSW::distance(a, b) -> Option<f32>"""
        out = C.c_float()
        rc = self._L.hnsw_distance(self._h, int(a), int(b), C.byref(out))
        return None if rc != _lib.OK else np.float32(out.value)

    def get_point(self, node):
        """HNSW::get_point(id) -> Option<&Point>"""
        if node < 0 or node >= self.len():
            return None
        return Point(self, int(node))

    def nb_layers(self):
        return int(self._L.hnsw_layer_count(self._h))

    def get_layer(self, layer_nb):
        if layer_nb >= self.nb_layers():
            raise HnswError(_lib.ERR_ARG, "Layer %d not found in the structure." % layer_nb)
        return Graph(self, layer_nb)

    def iter_layers(self):
        return [Graph(self, l) for l in range(self.nb_layers())]

    def assert_param_compliance(self):
        ok = C.c_int()
        check(self._L.hnsw_check_param_compliance(self._h, C.byref(ok)))
        return bool(ok.value)

    # ---- persistence ------------------------------------------------------------------------------
    def save(self, path):
        check(self._L.hnsw_save(self._h, str(path).encode()))

    @staticmethod
    def load(path):
        L = _lib.lib()
        h = C.c_void_p()
        check(L.hnsw_load(str(path).encode(), C.byref(h)))
        p = Params()
        check(L.hnsw_get_params(h, C.byref(p)))
        return HNSW(h, int(p.dim), int(p.vec_kind))

    # ---- device -------------------------------------------------------------------------------------
    def set_device(self, device):
        check(self._L.hnsw_set_device(self._h, int(device)))

    def set_option(self, key, value):
        check(self._L.hnsw_set_option(self._h, key.encode(), int(value)))

    def upload(self):
        check(self._L.hnsw_upload(self._h))

    def device_bytes(self):
        b = C.c_uint64()
        check(self._L.hnsw_device_bytes(self._h, C.byref(b)))
        return b.value

    def stat(self, key):
        """hnsw_get_stat: "uploads", "point_patches", "patch_fallbacks", "coalesced_batches", "coalesced_queries",
        "coalesced_max_batch", "deleted", "deleted_mask_words_uploaded", "deleted_queries_graph", ... (the header) """
        b = C.c_uint64()
        check(self._L.hnsw_get_stat(self._h, key.encode(), C.byref(b)))
        return b.value

    def batch_threads(self, Q, nq, n, ef, callers, calls):
        """hnsw_bench_batch_threads: `callers` host threads x `calls` hnsw_search_batch calls of nq queries each (host
        pointers in and out); -> queries per second over all callers"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be total x %d" % self.dim)
        wall = C.c_double()
        check(self._L.hnsw_bench_batch_threads(self._h, _p(Q, _f32p), Q.shape[0], int(nq), n, ef, int(callers), int(calls),
                                               C.byref(wall)))
        return callers * calls * nq / wall.value

    def search_threads(self, Q, n, ef, threads, seconds):
        """The reference's call pattern as a load (hnsw_bench_search_threads): `threads` host threads, each blocked in
        its own one-query hnsw_search call.  -> (ids [nq, n], counts [nq], calls, wall seconds,
        {p50, p90, p99, max, mean} latency in us + cpu_user_s / cpu_sys_s of the process over the run)"""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise HnswError(_lib.ERR_BAD_DIM, "queries must be nq x %d" % self.dim)
        nq = Q.shape[0]
        ids = np.full((nq, max(n, 1)), _lib.UINT32_MAX, dtype=np.uint32)
        counts = np.zeros(nq, dtype=np.uint32)
        calls, wall = C.c_uint64(), C.c_double()
        lat = (C.c_double * 7)()
        check(self._L.hnsw_bench_search_threads(self._h, _p(Q, _f32p), nq, n, ef, int(threads), float(seconds),
                                                _p(ids, _u32p), _p(counts, _u32p), C.byref(calls), C.byref(wall), lat))
        return ids[:, :n], counts, calls.value, wall.value, dict(zip(("p50", "p90", "p99", "max", "mean", "cpu_user_s", "cpu_sys_s"), list(lat)))

    # ---- replication over the GPUs of a node ------------------------------------
    @staticmethod
    def replicate(index, m, ef_cons, dim, vec_kind, group=None, src=0, device=None, chunk_bytes=1 << 30):
        """Every rank of the torch.distributed group calls this; `index` is the built index on rank `src`
        (ignored elsewhere).  The snapshot's flat HBM arrays are broadcast from `src` -- RCCL over xGMI when
        the group's backend is nccl, staged through the host for gloo (the CPU tests) -- and every other
        rank gets a device-only replica that answers searches (hnsw_snapshot_describe / _adopt / _commit).
        Returns the source's own index on `src`, the replica elsewhere.  Arrays travel in pieces of at most
        chunk_bytes: a 51-GB row table is not one collective."""
        import torch
        import torch.distributed as dist
        from ._lib import SnapshotDesc
        rank = dist.get_rank(group)
        on_device = dist.get_backend(group) == "nccl"
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        L = _lib.lib()
        desc = SnapshotDesc()
        if rank == src:
            index.set_device(dev.index if dev.index is not None else 0)
            check(L.hnsw_snapshot_describe(index._h, C.byref(desc)))
            out = index
        else:
            out = HNSW.new(m, ef_cons, dim, vec_kind)
            out.set_device(dev.index if dev.index is not None else 0)
        # sizes + header: 7 + 32 words, one small broadcast
        meta = torch.zeros(7 + 32, dtype=torch.int64)
        if rank == src:
            meta[:7] = torch.tensor([int(desc.bytes[i]) for i in range(7)], dtype=torch.int64)
            meta[7:] = torch.tensor([int(desc.header[i]) for i in range(32)], dtype=torch.int64)
        meta = meta.to(dev) if on_device else meta
        dist.broadcast(meta, src=src, group=group)
        meta = meta.cpu()
        if rank != src:
            for i in range(7):
                desc.bytes[i] = int(meta[i])
            for i in range(32):
                desc.header[i] = int(meta[7 + i])
            check(L.hnsw_snapshot_adopt(out._h, C.byref(desc)))

        class _Mem:  # a view of library-owned device memory for torch (CUDA array interface)
            def __init__(self, ptr, nbytes):
                self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

        for i in range(7):
            nbytes = int(desc.bytes[i])
            if nbytes == 0:
                continue
            whole = torch.as_tensor(_Mem(int(desc.ptr[i]), nbytes), device=dev)
            for lo in range(0, nbytes, chunk_bytes):
                piece = whole[lo:min(nbytes, lo + chunk_bytes)]
                if on_device:
                    dist.broadcast(piece, src=src, group=group)
                else:
                    host = piece.cpu() if rank == src else torch.empty(piece.shape[0], dtype=torch.uint8)
                    dist.broadcast(host, src=src, group=group)
                    if rank != src:
                        piece.copy_(host)
        torch.cuda.synchronize(dev)
        if rank != src:
            check(L.hnsw_snapshot_commit(out._h))
        return out


class MaskSet:
    """hnsw_mask_set: n_masks allow-lists of allow_bits bits that live with an index (HNSW.mask_set makes one).  Managing
    it needs no GPU; the next search that names it brings its HBM copy up to date.  Keeps its index alive; close() (or
    garbage collection) frees it."""

    def __init__(self, index, handle):
        self._index = index
        self._L = index._L
        self._s = handle
        n, b = C.c_uint32(), C.c_uint64()
        check(self._L.hnsw_mask_set_info(self._s, C.byref(n), C.byref(b)))
        self.n_masks, self.allow_bits = n.value, b.value
        self._W = (self.allow_bits + 63) // 64

    def close(self):
        if getattr(self, "_s", None):
            self._L.hnsw_mask_set_free(self._s)
            self._s = None
            self._index = None

    __del__ = close

    def write(self, row, allow):
        """replaces a row: a bool array of allow_bits entries, an array of allowed ids, or W packed uint64 words"""
        a = np.asarray(allow)
        if a.dtype == np.uint64:
            words = np.ascontiguousarray(a.reshape(-1))
        else:
            words, bits = pack_allow(a, self.allow_bits)
            if bits != self.allow_bits:
                raise ValueError("a bool row has allow_bits = %d entries, got %d" % (self.allow_bits, bits))
        if words.shape[0] < self._W:
            raise ValueError("a row has %d words, got %d" % (self._W, words.shape[0]))
        check(self._L.hnsw_mask_set_write(self._s, int(row), _p(words, _u64p)))

    def update(self, row, ids, allow=True):
        """sets (allow) or clears the bits of `ids` in one row; an id >= allow_bits changes nothing and raises"""
        a = np.asarray(ids).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > _lib.UINT32_MAX):
            raise HnswError(_lib.ERR_ARG, "ids must be in [0, 2^32)")
        a = np.ascontiguousarray(a, dtype=np.uint32)
        check(self._L.hnsw_mask_set_update(self._s, int(row), _p(a, _u32p), a.shape[0], 1 if allow else 0))

    def read(self, row):
        """-> the row's W words (uint64)"""
        words = np.zeros(max(self._W, 1), dtype=np.uint64)
        check(self._L.hnsw_mask_set_read(self._s, int(row), _p(words, _u64p)))
        return words[: self._W]

    def count(self, row):
        """-> the row's set bits (below allow_bits; deleted ids are not taken out)"""
        c = C.c_uint64()
        check(self._L.hnsw_mask_set_count(self._s, int(row), C.byref(c)))
        return c.value


def pack_allow(allow, n_points=None):
    """-> (words uint64, allow_bits): the mask of hnsw_search_batch_filtered, id i at bit i & 63 of word i >> 6.
    allow: a bool array over ids (allow_bits = its length) or an integer array of allowed ids (allow_bits = n_points,
    or one past the largest id when n_points is None)."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        bits = a.reshape(-1)
    else:
        ids = a.reshape(-1).astype(np.int64)
        if ids.size and ids.min() < 0:
            raise ValueError("allowed ids must be non-negative")
        n = int(n_points) if n_points is not None else (int(ids.max()) + 1 if ids.size else 0)
        ids = ids[ids < n]
        bits = np.zeros(n, dtype=np.bool_)
        bits[ids] = True
    nbits = bits.shape[0]
    padded = np.zeros(((nbits + 63) // 64) * 64, dtype=np.bool_)
    padded[:nbits] = bits
    words = np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)
    if words.size == 0:
        words = np.zeros(1, dtype=np.uint64)
    return words, nbits


def pack_ranges(ranges, nq=None):
    """The range lists of a batch as hnsw_search_batch_filtered_ranges takes them -> (lo, hi), uint32 [nq, K], row-major.
    ranges: one list per query, its members (lo, hi) pairs or an int x meaning [x, x]; K is the longest list's length
    (at least 1) and shorter lists are padded with the empty range (1, 0)."""
    def member(x):
        if isinstance(x, (int, np.integer)):
            l = h = int(x)
        else:
            l, h = (int(v) for v in x)
        if not (0 <= l <= _lib.UINT32_MAX and 0 <= h <= _lib.UINT32_MAX):
            raise ValueError("range bounds are labels: in [0, 2^32)")
        return l, h
    rows = [[member(x) for x in r] for r in ranges]
    if nq is not None and len(rows) != nq:
        raise ValueError("one range list per query")
    K = max([len(r) for r in rows] + [1])
    lo = np.ones((len(rows), K), dtype=np.uint32)
    hi = np.zeros((len(rows), K), dtype=np.uint32)
    for i, r in enumerate(rows):
        for k, (l, h) in enumerate(r):
            lo[i, k], hi[i, k] = l, h
    return lo, hi


def pack_allow_many(masks, n_points=None):
    """-> (words [G, W] uint64, C-contiguous, allow_bits): the masks of hnsw_search_batch_filtered_multi.  masks: a 2-D
    bool array [G, bits], or a sequence whose items are each what pack_allow takes (bool arrays of one common length,
    or id arrays); row g is pack_allow(masks[g], n_points)[0] word for word."""
    packed = [pack_allow(m, n_points) for m in masks]
    if not packed:
        raise ValueError("pack_allow_many needs at least one mask")
    bits = {b for _, b in packed}
    if len(bits) != 1:
        raise ValueError("the masks of one call share allow_bits: got %s" % sorted(bits))
    return np.ascontiguousarray(np.stack([w for w, _ in packed])), bits.pop()


def synth_rows(recipe, seed, first_row, n, d, nb_threads=8):
    out = np.zeros((n, d), dtype=np.float32)
    check(_lib.lib().hnsw_synth_rows(recipe, seed, first_row, n, d, _p(out, _f32p), nb_threads))
    return out


def draw_levels(m, n):
    out = np.zeros(n, dtype=np.uint8)
    check(_lib.lib().hnsw_draw_levels(m, n, _p(out, _u8p)))
    return out


def device_count():
    c = C.c_int()
    check(_lib.lib().hnsw_device_count(C.byref(c)))
    return c.value


def kernel_name(name):
    """the kernel launch log's name for a kernel symbol (mangled or not): hnsw_kernel_name"""
    raw = name.encode() if isinstance(name, str) else name
    need = C.c_uint64()
    check(_lib.lib().hnsw_kernel_name(raw, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(_lib.lib().hnsw_kernel_name(raw, buf, need.value, C.byref(need)))
    return buf.value.decode()


class KernelLog(dict):
    """{kernel instantiation name: launches} recorded while the `kernel_log()` block ran (a test seam)"""


@contextlib.contextmanager
def kernel_log():
    """Record every kernel launch of the process for the duration of the block:

        with H.kernel_log() as log:
            index.search_batch(Q, 10, 64)
        assert set(log) == {"hx_lean_f32_kernel<100, Lst<1>, 4>"}

    The log is process-wide (launches from other threads count too) and is filled in when the block ends."""
    L = _lib.lib()
    log = KernelLog()
    check(L.hnsw_kernel_log(1))
    try:
        yield log
    finally:
        check(L.hnsw_kernel_log(0))
        need = C.c_uint64()
        check(L.hnsw_kernel_log_get(None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        check(L.hnsw_kernel_log_get(buf, need.value, C.byref(need)))
        for line in buf.value.decode().splitlines():
            name, _, count = line.rpartition(" ")
            log[name] = int(count)
