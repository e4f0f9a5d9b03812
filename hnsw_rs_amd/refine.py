"""Refined search (include/hnsw_mi355x.h, "refined search"): a candidate list re-scored against a table of full rows --
float32, or float16 widened exactly -- and cut to the nearest, restated in numpy float32, and the row table that keeps
such rows in HBM beside an index.  The library's own forms run on the device (HNSW.search_batch_refined, refine_device);
refine_lists is what they are held to, bit for bit, and what a caller without a GPU at hand can use on lists it already
has."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

DTYPES = {"f32": _lib.ROWS_F32, "f16": _lib.ROWS_F16, "float32": _lib.ROWS_F32, "float16": _lib.ROWS_F16,
          _lib.ROWS_F32: _lib.ROWS_F32, _lib.ROWS_F16: _lib.ROWS_F16}
NP_DTYPE = {_lib.ROWS_F32: np.float32, _lib.ROWS_F16: np.float16}


def dtype_of(dtype):
    """"f32" / "f16" (or a numpy dtype, or ROWS_F32 / ROWS_F16) -> the ABI's dtype word"""
    try:
        return DTYPES[dtype]
    except (KeyError, TypeError):
        pass
    try:
        return DTYPES[np.dtype(dtype).name]
    except (KeyError, TypeError):
        raise ValueError("dtype is 'f32' or 'f16'")


def refine_lists(Qfull, ids_in, counts, statuses, table, n_out):
    """THE REFINEMENT of include/hnsw_mi355x.h.  Qfull [nq, full_dim] float32, ids_in [nq, pool] uint32, counts [nq] or
    None (an entry is then present iff its id is not UINT32_MAX), statuses [nq] or None (all OK), table [rows, full_dim]
    float32 or float16 (widened exactly).  A query whose status is not OK keeps it; else a present id at or beyond the
    table's rows gives ERR_ARG (no row is read for that query); else a NaN element of its full row gives ERR_NAN_INPUT.
    Such a query has count 0 and padded rows.  Otherwise the distance of a present entry is sqrt(s), s = 0, then
    t = row[e] - q[e]; s = s + t * t over the elements in order, every operation in float32 (the loop below is sequential
    over the elements and vectorised over the candidates); the present entries are ranked by (distance bits, id), a NaN
    distance is never returned, duplicate ids are separate entries, and the n_out best are returned.
    -> ids [nq, n_out] (pad UINT32_MAX), dists [nq, n_out] (pad +inf), counts [nq], statuses [nq]"""
    Qfull = np.ascontiguousarray(Qfull, dtype=np.float32)
    ids_in = np.ascontiguousarray(ids_in, dtype=np.uint32)
    table = np.asarray(table)
    if table.dtype not in (np.float32, np.float16):
        raise ValueError("the table is float32 or float16")
    if Qfull.ndim != 2 or ids_in.ndim != 2 or table.ndim != 2 or ids_in.shape[0] != Qfull.shape[0] or \
            table.shape[1] != Qfull.shape[1]:
        raise ValueError("Qfull is [nq, full_dim], ids_in [nq, pool] and the table [rows, full_dim]")
    nq, pool = ids_in.shape
    full_dim, n_out = Qfull.shape[1], int(n_out)
    if not 1 <= n_out <= pool <= _lib.REFINE_POOL_MAX or not 1 <= full_dim <= _lib.REFINE_MAX_DIM:
        raise ValueError("1 <= n_out <= pool <= %d and 1 <= full_dim <= %d" % (_lib.REFINE_POOL_MAX, _lib.REFINE_MAX_DIM))
    if counts is not None:
        counts = np.asarray(counts).reshape(nq)
    st_in = np.zeros(nq, dtype=np.int64) if statuses is None else np.array(statuses, dtype=np.int64).reshape(nq)
    o_ids = np.full((nq, n_out), _lib.UINT32_MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    o_status = st_in.copy()
    j = np.arange(pool)
    for q in range(nq):
        if st_in[q] != _lib.OK:
            continue
        present = ids_in[q] != _lib.UINT32_MAX if counts is None else j < min(int(counts[q]), pool)
        cand = ids_in[q][present]  # in list order, duplicates kept
        if (cand.astype(np.int64) >= table.shape[0]).any():
            o_status[q] = _lib.ERR_ARG
            continue
        if np.isnan(Qfull[q]).any():
            o_status[q] = _lib.ERR_NAN_INPUT
            continue
        if cand.size == 0:
            continue
        rows = np.ascontiguousarray(table[cand].astype(np.float32).T)  # [full_dim, c]: an element of every candidate
        s = np.zeros(cand.size, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for e in range(full_dim):  # one left-to-right chain per candidate
                t = rows[e] - Qfull[q, e]
                s = s + t * t
            d = np.sqrt(s)
        assert d.dtype == np.float32
        live = np.flatnonzero(~np.isnan(d))
        order = live[np.lexsort((cand[live], d[live].view(np.uint32)))][:n_out]
        k = order.size
        o_ids[q, :k], o_dists[q, :k], o_counts[q] = cand[order], d[order], k
    return o_ids, o_dists, o_counts, o_status


def f32_to_f16(values):
    """hnsw_f32_to_f16: float32 values rounded to IEEE binary16, to nearest and ties to even, as the library's row table
    rounds them -> uint16 bits of the same shape.  A NaN, or a value that rounds to an infinity, raises (ERR_NAN_INPUT).
    Needs no GPU."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(v.shape, dtype=np.uint16)
    check(_lib.lib().hnsw_f32_to_f16(v.ctypes.data_as(_lib.f32p), v.size, out.ctypes.data_as(_lib.u16p)))
    return out


def refine_device(nq, pool, n_out, full_dim, dtype, d_table, table_rows, d_Qfull, d_ids_in, d_counts_in, d_stats_in, d_ids,
                  d_dists, d_counts=None, d_stats=None, stream=0):
    """hnsw_refine_device over torch device tensors (or raw device pointers): the [nq, pool] candidate ids a *_device
    search left (d_counts_in / d_stats_in [nq] or None), re-scored against d_table -- table_rows x full_dim elements of
    `dtype` ("f32" / "f16") -- with the full queries d_Qfull float32 [nq, full_dim], into d_ids / d_dists [nq, n_out]
    (/ d_counts / d_stats).  ONE launch enqueued on `stream` of the current device, no sync of it; needs no index."""
    from .hnsw import HNSW
    p = HNSW._dptr
    check(_lib.lib().hnsw_refine_device(
        nq, pool, n_out, full_dim, dtype_of(dtype), p(d_table), table_rows, p(d_Qfull), p(d_ids_in), p(d_counts_in),
        p(d_stats_in), p(d_ids), p(d_dists), p(d_counts), p(d_stats), stream or None))


class RowTable:
    """hnsw_row_table: full rows -- float32 or float16 -- that live in HBM beside an index, row id = index id
    (HNSW.row_table makes one).  The host keeps no copy; the table is not saved, cloned or replicated with the index
    (save and HNSW.load_row_table carry it in a file of its own).  Keeps its index alive; close() (or garbage collection) frees it."""

    def __init__(self, index, handle):
        self._index = index
        self._L = index._L
        self._t = handle
        d, k, r = C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(self._L.hnsw_row_table_info(self._t, C.byref(d), C.byref(k), C.byref(r)))
        self.full_dim, self.dtype = d.value, k.value

    def close(self):
        if getattr(self, "_t", None):
            self._L.hnsw_row_table_free(self._t)
            self._t = None
            self._index = None

    __del__ = close

    @property
    def rows(self):
        r = C.c_uint64()
        check(self._L.hnsw_row_table_info(self._t, None, None, C.byref(r)))
        return r.value

    def _block(self, rows, dtype):
        a = np.ascontiguousarray(rows, dtype=dtype)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != self.full_dim:
            raise _lib.HnswError(_lib.ERR_BAD_DIM, "rows must be n x %d" % self.full_dim)
        return a

    def write(self, first_id, rows):
        """rows [n, full_dim] (anything float32 can hold) to ids first_id .. first_id + n - 1; a float16 table rounds
        to nearest even.  A NaN, an infinity or a value that rounds to one changes nothing and raises; so does a hole."""
        a = self._block(rows, np.float32)
        check(self._L.hnsw_row_table_write(self._t, int(first_id), a.shape[0], a.ctypes.data_as(_lib.f32p)))

    def write_raw(self, first_id, rows):
        """the same with rows already in the table's dtype (float16 for a float16 table), copied as they are"""
        a = self._block(rows, NP_DTYPE[self.dtype])
        check(self._L.hnsw_row_table_write_raw(self._t, int(first_id), a.shape[0], C.c_void_p(a.ctypes.data)))

    def read(self, first_id, n):
        """-> rows first_id .. first_id + n - 1 as float32 [n, full_dim], widened exactly"""
        out = np.zeros((int(n), self.full_dim), dtype=np.float32)
        check(self._L.hnsw_row_table_read(self._t, int(first_id), int(n), out.ctypes.data_as(_lib.f32p)))
        return out

    def save(self, path):
        """the table into one file at `path` (hnsw_row_table_save: a big-endian header and the rows in the table's dtype,
        bit for bit); HNSW.load_row_table reads it back.  A table that was never written needs no GPU."""
        check(self._L.hnsw_row_table_save(self._t, str(path).encode()))

    def device(self):
        """-> (device pointer of the array in HBM or None before the first write, rows): what refine_device takes"""
        p, r = C.c_void_p(), C.c_uint64()
        check(self._L.hnsw_row_table_device(self._t, C.byref(p), C.byref(r)))
        return p.value, r.value
