"""Refined search on the host (include/hnsw_mi355x.h, "refined search"): the numpy restatement
(hnsw_rs_amd.refine.refine_lists) against a second, deliberately plain one (tests/refine_cases.py) bit for bit, the
library's binary16 rounding against numpy's, and everything hnsw_refine_device, hnsw_search_batch_refined and the row
table's calls decide before they touch a device -- every argument error with its message, nq == 0, the stat keys, the
exported symbols and their prototypes -- and the registers of the kernel that carries the new form.  None of this needs
a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import refine_cases as RC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p, u16p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
TABLE_SYMBOLS = ("hnsw_row_table_create", "hnsw_row_table_info", "hnsw_row_table_write", "hnsw_row_table_write_raw",
                 "hnsw_row_table_read", "hnsw_row_table_device", "hnsw_f32_to_f16")
NEW_SYMBOLS = ("hnsw_refine_device", "hnsw_search_batch_refined") + TABLE_SYMBOLS
KEYS = ("uploads", "refine_calls", "refine_launches", "row_table_writes")
POOLS = (1, 7, 64, 65, 1024)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("pool", POOLS)
def test_refine_lists_is_the_plain_loop_bit_for_bit(pool, dtype):
    full_dim = 5 if pool == 1024 else 9  # (the plain loop is one numpy scalar operation per step)
    table = RC.make_table(60, full_dim, dtype, 100 + pool)
    for with_counts in (True, False):
        Q, ids, counts, statuses = RC.make_case(RC.N_PLANTED + 2, pool, table, with_counts, 10 * pool + with_counts)
        for n_out in sorted({1, pool}):
            what = "pool=%d dtype=%d counts=%s n_out=%d" % (pool, dtype, with_counts, n_out)
            got = H.refine_lists(Q, ids, counts, statuses, table, n_out)
            want = RC.naive(Q, ids, counts, statuses, table, n_out)
            RC.assert_refined_equal(got, want, what)
            assert got[0].shape == got[1].shape == (len(Q), n_out) and got[1].dtype == np.float32
            RC.check_planted(got, pool, n_out, what)
            for q in range(len(Q)):  # sorted by (distance bits, id), no NaN, padded behind the count
                c = int(got[2][q])
                b, i = got[1][q, :c].view(np.uint32).astype(np.int64), got[0][q, :c].astype(np.int64)
                assert not np.isnan(got[1][q]).any(), what
                assert all(b[a] < b[a + 1] or (b[a] == b[a + 1] and i[a] <= i[a + 1]) for a in range(c - 1)), what
                assert (got[0][q, c:] == MAX).all() and np.isposinf(got[1][q, c:]).all(), what


def test_zero_counts_and_no_statuses():
    table = RC.make_table(40, 6, RC.F32, 3)
    Q, ids, _, _ = RC.make_case(RC.N_PLANTED, 7, table, True, 5)
    Q[RC.Q_NAN] = 0.5  # (not what this test is about)
    ids[RC.Q_BEYOND] = 20
    for fn in (H.refine_lists, RC.naive):
        got = fn(Q, ids, np.zeros(len(Q), dtype=np.uint32), None, table, 3)
        assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0] == MAX).all() and np.isposinf(got[1]).all()
        full = fn(Q, ids, None, None, table, 7)
        assert (full[3] == 0).all() and full[2][RC.Q_TWINS] == 7


def test_a_small_case_by_hand():
    table = np.array([[0, 0], [3, 4], [3, 4], [1, 0], [6, 8]], dtype=np.float32)
    Q = np.array([[0, 0]], dtype=np.float32)
    ids = np.array([[4, 2, 3, 1, MAX, 3]], dtype=np.uint32)
    for fn in (H.refine_lists, RC.naive):
        for t in (table, table.astype(np.float16)):
            got = fn(Q, ids, None, None, t, 6)
            assert got[0][0].tolist() == [3, 3, 1, 2, 4, MAX] and got[1][0].tolist() == [1, 1, 5, 5, 10, np.inf]
            assert got[2][0] == 5 and got[3][0] == 0
            got = fn(Q, ids, np.array([2]), None, t, 1)
            assert got[0][0].tolist() == [2] and got[1][0].tolist() == [5] and got[2][0] == 1


def test_refine_lists_refuses_shapes_beyond_the_limits():
    table = np.zeros((10, 4), dtype=np.float32)
    Q, ids = np.zeros((2, 4), dtype=np.float32), np.zeros((2, 8), dtype=np.uint32)
    for a in ((Q, ids, None, None, table, 0), (Q, ids, None, None, table, 9), (Q[:, :3], ids, None, None, table, 1),
              (Q, np.zeros((2, 1025), dtype=np.uint32), None, None, table, 1), (Q, ids[:1], None, None, table, 1),
              (Q, ids, None, None, table.astype(np.float64), 1),
              (np.zeros((2, 4097), dtype=np.float32), ids, None, None, np.zeros((3, 4097), dtype=np.float32), 1)):
        with pytest.raises(ValueError):
            H.refine_lists(*a)
    got = H.refine_lists(Q, np.zeros((2, 1024), dtype=np.uint32), None, None, table, 1024)
    assert got[2].tolist() == [1024, 1024]


# ---- the binary16 rounding ------------------------------------------------------------------------------------------------
def f16_sweep():
    """float32 values around everything binary16 rounding decides: every f16 value, the exact ties between neighbours
    (both ways: to the even neighbour below and above) and their float32 neighbours, the subnormal range, the edges"""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)  # every finite f16 >= 0, ascending
    ties = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)  # (exact: 12 bits)
    assert (ties.astype(np.float64) * 2 == h[:-1].astype(np.float64) + h[1:]).all()
    around = np.concatenate([np.nextafter(ties, np.float32(0)), ties, np.nextafter(ties, np.float32(np.inf))])
    tiny = np.array([0.0, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, 1e-45, 2.0 ** -24,
                     2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0))], dtype=np.float32)
    edge = np.array([65504.0, 65519.0, np.nextafter(np.float32(65520.0), np.float32(0))], dtype=np.float32)
    rng = np.random.default_rng(1)
    rnd = (rng.standard_normal(4000) * np.exp(rng.uniform(-20, 11, 4000))).astype(np.float32)
    rnd = rnd[np.abs(rnd) < 65519]
    v = np.concatenate([h, around, tiny, edge, rnd])
    return np.concatenate([v, -v])


def test_f32_to_f16_is_numpys_rounding():
    v = f16_sweep()
    want = v.astype(np.float16)
    assert np.isfinite(want).all() and len(v) > 200000
    got = H.f32_to_f16(v)
    assert got.dtype == np.uint16 and np.array_equal(got, want.view(np.uint16))
    # ties both ways, the subnormals and the edges are in it
    assert H.f32_to_f16(np.float32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])).tolist() == [0x3C00, 0x3C02]
    assert H.f32_to_f16(np.float32([2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, -0.0, 65504, -65504, 65519.996])).tolist() == \
        [0, 1, 2, 0x8000, 0x7BFF, 0xFBFF, 0x7BFF]


def test_f32_to_f16_refuses_what_rounds_to_infinity_and_nan():
    L = _lib.lib()
    for bad in (65520.0, -65520.0, 1e10, np.inf, -np.inf, np.nan):
        v = np.array([1.0, bad, 2.0], dtype=np.float32)
        out = np.full(3, 0x1234, dtype=np.uint16)
        assert L.hnsw_f32_to_f16(ptr(v, f32p), 3, ptr(out, u16p)) == _lib.ERR_NAN_INPUT, bad
        assert L.hnsw_last_error() == b"f32 to f16: value 1 is a NaN or rounds to an infinity; nothing is written"
        assert (out == 0x1234).all()
        with pytest.raises(H.HnswError) as e:
            H.f32_to_f16(v)
        assert e.value.code == _lib.ERR_NAN_INPUT
    assert L.hnsw_f32_to_f16(None, 3, None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"f32 to f16: needs the values and a place for the halves"
    assert L.hnsw_f32_to_f16(None, 0, None) == _lib.OK


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(nq=6, pool=16, n_out=10, full_dim=32, dtype=0, table=fake, rows=100, Q=fake, i_in=fake, c_in=fake, s_in=fake,
             ids=fake, dists=fake, counts=fake, stats=fake):
        return L.hnsw_refine_device(nq, pool, n_out, full_dim, dtype, table, rows, Q, i_in, c_in, s_in, ids, dists, counts,
                                    stats, None)

    for kw in (dict(pool=0), dict(n_out=0), dict(n_out=17), dict(pool=1025, n_out=1), dict(pool=0x80000000, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"refine: needs 1 <= n_out <= pool <= 1024", kw
    for kw in (dict(full_dim=0), dict(full_dim=4097)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"refine: needs 1 <= full_dim <= 4096", kw
    for dtype in (2, 7, 0xFFFFFFFF):
        assert call(dtype=dtype) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"refine: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)"
    assert call(pool=1024, n_out=1024, full_dim=4096, dtype=1, table=None) == _lib.ERR_ARG  # (within the limits: the pointer)
    assert b"needs the table" in L.hnsw_last_error()
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refine: at most 2^31 - 1 queries"
    for name in ("table", "Q", "i_in", "ids", "dists"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == \
            b"refine: needs the table, the full queries, the candidates' ids and the id and distance outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refine: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # the order of the checks: the shape before nq, nq before the pointers, the pointers before the stats pair
    assert call(pool=0, nq=1 << 31, table=None, stats=None) == _lib.ERR_ARG and b"n_out <= pool" in L.hnsw_last_error()
    assert call(nq=1 << 31, table=None, stats=None) == _lib.ERR_ARG and b"2^31 - 1" in L.hnsw_last_error()
    assert call(table=None, stats=None) == _lib.ERR_ARG and b"needs the table" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, pool=0, n_out=0, full_dim=0, dtype=9, table=None, Q=None, i_in=None, ids=None, dists=None, stats=None) == _lib.OK
    with pytest.raises(H.HnswError) as e:
        H.refine_device(4, 10, 11, 32, "f32", 256, 100, 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        H.refine_device(4, 10, 5, 32, "bf16", 256, 100, 256, 256, None, None, 256, 256)
    H.HNSW.refine_device(0, 10, 5, 32, "f16", None, 0, None, None, None, None, None, None)  # nq == 0


def test_row_table_argument_errors_need_no_device():
    index = small()
    L = _lib.lib()
    t = C.c_void_p()
    assert L.hnsw_row_table_create(None, 8, 0, C.byref(t)) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"row table: needs a handle and a place for the table"
    assert L.hnsw_row_table_create(index._h, 8, 0, None) == _lib.ERR_ARG
    for full_dim in (0, 4097):
        assert L.hnsw_row_table_create(index._h, full_dim, 0, C.byref(t)) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"row table: needs 1 <= full_dim <= 4096"
    assert L.hnsw_row_table_create(index._h, 8, 2, C.byref(t)) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"row table: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)"
    assert not t.value
    with pytest.raises(ValueError):
        index.row_table(8, "bf16")
    for dtype, np_dtype in (("f32", np.float32), ("f16", np.float16)):
        tab = index.row_table(8, dtype)
        assert (tab.full_dim, tab.dtype, tab.rows) == (8, H.ROWS_F16 if dtype == "f16" else H.ROWS_F32, 0)
        assert tab.device() == (None, 0)
        rows = np.ones((3, 8), dtype=np.float32)
        assert L.hnsw_row_table_write(None, 0, 3, ptr(rows, f32p)) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"row table: needs a table and the rows to write"
        assert L.hnsw_row_table_write(tab._t, 0, 3, None) == _lib.ERR_ARG
        assert L.hnsw_row_table_write_raw(tab._t, 0, 3, None) == _lib.ERR_ARG
        assert L.hnsw_row_table_write(tab._t, 0, 0, None) == _lib.OK  # nothing to write
        assert L.hnsw_row_table_write(tab._t, 1, 3, ptr(rows, f32p)) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"row table: a write at id 1 would leave a hole behind its 0 rows"
        assert L.hnsw_row_table_write_raw(tab._t, 2, 1, ptr(rows, f32p)) == _lib.ERR_ARG
        assert b"would leave a hole" in L.hnsw_last_error()
        assert L.hnsw_row_table_write(tab._t, 0, 1 << 32, ptr(rows, f32p)) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"row table: at most 2^32 - 1 rows"
        for bad in (np.nan, np.inf, -np.inf) + ((65520.0,) if dtype == "f16" else ()):
            rows[1, 5] = bad
            with pytest.raises(H.HnswError) as e:
                tab.write(0, rows)
            assert e.value.code == _lib.ERR_NAN_INPUT
            assert str(e.value).endswith("row table: row 1 holds a NaN or a value beyond the dtype's range; nothing is written")
            if np.isfinite(bad):
                continue
            with pytest.raises(H.HnswError) as e:
                tab.write_raw(0, rows.astype(np_dtype))
            assert e.value.code == _lib.ERR_NAN_INPUT
        with pytest.raises(H.HnswError) as e:
            tab.write(0, np.ones((2, 7), dtype=np.float32))
        assert e.value.code == _lib.ERR_BAD_DIM
        with pytest.raises(H.HnswError) as e:
            tab.read(0, 1)
        assert e.value.code == _lib.ERR_ARG and "rows 0 .. 1 of 0" in str(e.value)
        assert tab.read(0, 0).shape == (0, 8)
        assert L.hnsw_row_table_read(None, 0, 0, None) == _lib.ERR_ARG
        assert L.hnsw_row_table_info(None, None, None, None) == _lib.ERR_ARG
        assert L.hnsw_row_table_device(None, None, None) == _lib.ERR_ARG
        assert L.hnsw_row_table_device(tab._t, None, None) == _lib.ERR_ARG
        assert tab.rows == 0 and tab.device() == (None, 0)
        tab.close()
        tab.close()
    L.hnsw_row_table_free(None)
    assert index.stat("row_table_writes") == 0 and index.stat("uploads") == 0


def test_search_argument_errors_need_no_device():
    index = small()
    other = small(n=50)
    FD = 20
    tab, foreign, narrow = index.row_table(FD, "f16"), other.row_table(FD, "f16"), index.row_table(D - 1, "f32")
    Q, Qf = rand_vectors(6, D, 12), rand_vectors(6, FD, 13)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    lo, hi = np.zeros(6, dtype=np.uint32), np.full(6, 5, dtype=np.uint32)

    def rc(h=index, t=tab, Q=Q, Qf=Qf, nq=6, n=4, pool=20, ef=32, s=None, mask_of=None, lo=None, hi=None, ids="own"):
        o_i = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_d, o_c = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_refined(None if h is None else h._h, None if t is None else t._t, ptr(Q, f32p), ptr(Qf, f32p),
                                           nq, n, pool, ef, s, ptr(mask_of, u32p), ptr(lo, u32p), ptr(hi, u32p), ptr(o_i, u32p),
                                           ptr(o_d, f32p), ptr(o_c, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_d == 3.5).all() and (o_c == 9).all() and (o_i is None or (o_i == 7).all())
        return code

    assert rc(h=None) == _lib.ERR_ARG
    assert rc(lo=lo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: a label range needs lo and hi, both or neither"
    assert rc(mask_of=lo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: mask_of needs its mask set"
    assert rc(t=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: needs a row table"
    assert rc(t=foreign) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: the row table belongs to another handle"
    for kw in (dict(pool=0), dict(n=0), dict(n=21), dict(pool=1025)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"refined search: needs 1 <= n <= pool <= 1024", kw
    assert rc(pool=65, lo=lo, hi=hi) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: needs pool <= 64 under a filter or while ids are deleted"
    assert rc(Qf=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: needs the full queries, an id buffer and at most 2^31 - 1 queries"
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(nq=1 << 31) == _lib.ERR_ARG
    assert b"2^31 - 1 queries" in L.hnsw_last_error()
    assert rc(t=narrow, Q=None, Qf=Qf[:, :D - 1].copy()) == _lib.ERR_ARG
    assert L.hnsw_last_error() == \
        b"refined search: without Q the index's queries are the first 12 elements of a full row, which has 11"
    assert rc() == _lib.ERR_ARG  # the table is empty: it does not cover the index
    assert L.hnsw_last_error() == b"refined search: the row table has 0 rows, the index 700"
    assert rc(Q=None) == _lib.ERR_ARG and b"has 0 rows" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle and the filter's own refusals)
    assert rc(nq=0) == _lib.OK and rc(nq=0, t=None, Q=None, Qf=None, ids=None, pool=0, n=0) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    # the candidate call's limit while ids are deleted
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65, n=4) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"refined search: needs pool <= 64 under a filter or while ids are deleted"
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty, t=empty.row_table(FD)) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    tab = index.row_table(20, "f32")
    Q, Qf = rand_vectors(6, D, 12), rand_vectors(6, 20, 13)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_refined(tab, Q, Qf[:, :5], 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:
        index.search_batch_refined(tab, Q[:, :5], Qf, 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:
        index.search_batch_refined(tab, Q[:4], Qf, 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_refined(tab, Q, Qf, 3, 10, 32, lo=1)
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_refined(tab, Q, Qf, 11, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_refined(tab, Q[:0], Qf[:0], 3, 10, 32)  # nq == 0
    assert got[0].shape == got[1].shape == (0, 3) and got[2].shape == (0,) and got[3].shape == (0, 4)
    got = index.search_batch_refined(tab, None, Qf[:0], 3, 10, 32)
    assert got[0].shape == (0, 3)
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("refine_calls", "refine_launches", "row_table_writes"):
        assert index.stat(key) == 0


def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers d_*, the stream, the handle,
    the table and the mask set are bound as void pointers)"""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if kind == "void**" or kind == "hnsw_row_table**":
        return C.POINTER(C.c_void_p)
    if name.startswith("d_") or kind in ("void*", "hnsw_index*", "hnsw_row_table*", "hnsw_mask_set*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint16_t*": u16p, "uint64_t*": C.POINTER(C.c_uint64),
            "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "float": C.c_float,
            "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS + ("hnsw_row_table_free",):
        assert hasattr(L, name), name
        m = re.search(r"^(int|void) %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is (C.c_int if m.group(1) == "int" else None), name
        assert [c_type_of(p) for p in params] == argtypes, name
    assert len(_lib.SYMBOLS["hnsw_refine_device"][1]) == 16 and len(_lib.SYMBOLS["hnsw_search_batch_refined"][1]) == 16
    for define, value in (("HNSW_ROWS_F32", H.ROWS_F32), ("HNSW_ROWS_F16", H.ROWS_F16),
                          ("HNSW_REFINE_POOL_MAX", H.REFINE_POOL_MAX), ("HNSW_REFINE_MAX_DIM", H.REFINE_MAX_DIM)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert (H.ROWS_F32, H.ROWS_F16, H.REFINE_POOL_MAX, H.REFINE_MAX_DIM) == (0, 1, 1024, 4096)
    assert "THE REFINEMENT" in header
    for words in ("NOT saved by hnsw_save", "NOT\n * cloned by hnsw_clone", "NOT part of the snapshot exchange"):
        assert words in header, words
    for method in ("row_table", "search_batch_refined", "refine_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.refine_lists) and callable(H.refine_device) and callable(H.f32_to_f16)


# ---- the kernel that carries the new form ------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernel_carries_the_refinement_without_scratch_or_vgpr_spills(tmp_path):
    """exact_scan.hip compiled for gfx950 with the Makefile's flags: the refinement is a source form of
    hx_distance_kernel, whose two instantiations stay the only ones and run without scratch and without spilled vector
    registers"""
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "exact_scan.hip")
    text = open(src).read()
    assert "refine_lists(dv, smem, lane)" in text, "the refinement is a source form of hx_distance_kernel"
    assert len(re.findall(r"__global__", text)) == 2, "no kernel was added beside the two"
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "exact_scan.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    seam = {k: v for k, v in kernels.items() if "hx_distance_kernel" in k}
    assert len(seam) == 2 and sum("ILi0E" in k for k in seam) == 1 and sum("ILi1E" in k for k in seam) == 1, sorted(kernels)
    for name, r in seam.items():
        assert "ScratchSize" in r and "VGPRs Spill" in r, (name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r.get("VGPRs", 0) <= 256, (name, r)
