"""Boosted search on the host (include/hnsw_mi355x.h, "boosted search"): the numpy restatement
(hnsw_rs_amd.boost.boost_lists) against a second, deliberately plain one (tests/boost_cases.py) bit for bit, known answers
worked out by hand, and everything hnsw_boost_device, hnsw_search_batch_boosted, hnsw_row_table_save and
hnsw_row_table_load decide before they touch a device -- every argument error with its message, nq == 0, the stat keys,
the exported symbols and their prototypes, the file of an empty table and every corrupt file -- and the registers of the
kernel that carries the new form.  None of this needs a GPU."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import boost_cases as BC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N, D = 300, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p, u16p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
NEW_SYMBOLS = ("hnsw_boost_device", "hnsw_search_batch_boosted", "hnsw_row_table_save", "hnsw_row_table_load")
KEYS = ("uploads", "boost_calls", "boost_launches", "row_table_writes")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the ABI: this test fails without the feature --------------------------------------------------------------------------
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
    return {"float*": f32p, "uint32_t*": u32p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "char*": C.c_char_p,
            "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        m = re.search(r"^(int|void) %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int, name
        assert [c_type_of(p) for p in params] == argtypes, name
    assert len(_lib.SYMBOLS["hnsw_boost_device"][1]) == 19 and len(_lib.SYMBOLS["hnsw_search_batch_boosted"][1]) == 18
    for define, value in (("HNSW_BOOST_POOL_MAX", H.BOOST_POOL_MAX), ("HNSW_BOOST_MAX_ATTRS", H.BOOST_MAX_ATTRS)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert (H.BOOST_POOL_MAX, H.BOOST_MAX_ATTRS) == (1024, 32)
    assert "THE BOOST" in header and "DROPS the entry" in header
    for method in ("search_batch_boosted", "boost_device", "load_row_table"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.boost_lists) and callable(H.boost_device) and callable(H.RowTable.save)


def test_stat_keys_exist():
    index = small(n=50)
    assert index.stat("boost_calls") == 0
    index.stat("boost_launches")  # (includes the handle-free primitive's launches of the whole process)


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BC.DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("n_attrs", BC.ATTRS)
@pytest.mark.parametrize("pool", BC.POOLS)
def test_boost_lists_is_the_plain_loop_bit_for_bit(pool, n_attrs, dtype):
    table = BC.make_table(60, n_attrs, dtype, 100 + pool + n_attrs)
    # (the plain loop is one numpy scalar operation per step: the widest shapes take one pairing of the two switches)
    variants = ((True, True), (False, False)) if pool * n_attrs > 8192 else ((True, True), (False, False), (True, False), (False, True))
    for with_counts, per_query in variants:
        ids, dists, counts, statuses, w = BC.make_case(pool, table, with_counts, per_query, 10 * pool + with_counts)
        n_outs = sorted({1, pool})
        want = BC.naive(ids, dists, counts, statuses, table, w, n_outs)
        for n_out in n_outs:
            what = "pool=%d A=%d dtype=%d counts=%s per_query=%s n_out=%d" % (pool, n_attrs, dtype, with_counts, per_query, n_out)
            got = H.boost_lists(ids, dists, counts, statuses, table, w, n_out)
            BC.assert_boosted_equal(got, want[n_out], what)
            assert got[0].shape == got[1].shape == got[2].shape == (BC.NQ, n_out) and got[1].dtype == np.float32
            BC.check_planted(got, ids, dists, table, pool, n_out, per_query, what)


def test_zero_counts_and_no_statuses():
    table = BC.make_table(40, 3, BC.F32, 3)
    ids, dists, _, _, w = BC.make_case(7, table, True, False, 5)
    ids[BC.Q_BEYOND] = 20
    zero = np.zeros(len(ids), dtype=np.uint32)
    for got in (H.boost_lists(ids, dists, zero, None, table, w, 3), BC.naive(ids, dists, zero, None, table, w, [3])[3]):
        assert (got[3] == 0).all() and (got[4] == 0).all() and (got[0] == MAX).all()
        assert np.isposinf(got[1]).all() and np.isposinf(got[2]).all()
    full = H.boost_lists(ids, dists, None, None, table, w, 7)
    assert (full[4] == 0).all() and full[3][BC.Q_TWINS] == 7


# ---- known answers, by hand ----------------------------------------------------------------------------------------------
def both(ids, dists, counts, statuses, table, w, n_out):
    """the two restatements' answers, which must agree"""
    got = H.boost_lists(ids, dists, counts, statuses, table, w, n_out)
    BC.assert_boosted_equal(got, BC.naive(np.asarray(ids, dtype=np.uint32), np.asarray(dists, dtype=np.float32), counts, statuses,
                                          np.asarray(table), w, [n_out])[n_out], "by hand")
    return got


def test_by_hand_newer_and_popular_beat_nearer():
    """attributes (age in days, popularity); w = (1, 0.5, -2): s = d + age / 2 - 2 * popularity, all exact in f32
         id 0: d 1.0, age 10, pop 1 -> 1 + 5 - 2   =  4
         id 1: d 2.0, age  0, pop 3 -> 2 + 0 - 6   = -4
         id 2: d 3.0, age  2, pop 0 -> 3 + 1 - 0   =  4   (ties with id 0: the id decides)
         id 3: d 0.5, age 40, pop 0 -> 0.5 + 20    = 20.5
       and the pad in the middle is no entry"""
    table = np.array([[10, 1], [0, 3], [2, 0], [40, 0]], dtype=np.float32)
    ids = np.array([[3, 2, MAX, 0, 1]], dtype=np.uint32)
    dists = np.array([[0.5, 3.0, 9.0, 1.0, 2.0]], dtype=np.float32)
    w = np.array([1, 0.5, -2], dtype=np.float32)
    for t in (table, table.astype(np.float16)):
        got = both(ids, dists, None, None, t, w, 5)
        assert got[0][0].tolist() == [1, 0, 2, 3, MAX] and got[1][0].tolist() == [-4, 4, 4, 20.5, np.inf]
        assert got[2][0].tolist() == [2, 1, 3, 0.5, np.inf] and got[3][0] == 4 and got[4][0] == 0
        got = both(ids, dists, np.array([2]), None, t, w, 1)  # with counts the first two entries alone
        assert got[0][0].tolist() == [2] and got[1][0].tolist() == [4] and got[2][0].tolist() == [3] and got[3][0] == 1


def test_by_hand_a_fused_multiply_add_would_round_otherwise():
    """w = (1, 1 + 2^-12), d = -1, a = 1 + 2^-12.  The product is 1 + 2^-11 + 2^-24: a tie between 1 + 2^-11 (even) and
    1 + 2^-11 + 2^-23, so the rounded product is 1 + 2^-11 and s = -1 + (1 + 2^-11) = 2^-11.  A fused multiply-add keeps
    the product whole and gives 2^-11 + 2^-24.  The second entry has exactly that larger score without any rounding
    (w[0] * d = 2^-11 + 2^-24 with a = 0), so it must rank BEHIND the first, not tie with it and win by its smaller id."""
    x = np.float32(1 + 2.0 ** -12)
    table = np.array([[0], [x]], dtype=np.float32)
    ids = np.array([[1, 0]], dtype=np.uint32)
    dists = np.array([[-1, 2.0 ** -11 + 2.0 ** -24]], dtype=np.float32)
    w = np.array([1, x], dtype=np.float32)
    assert float(x) * float(x) == 1 + 2.0 ** -11 + 2.0 ** -24  # (exact in a double: the tie)
    got = both(ids, dists, None, None, table, w, 2)
    assert got[0][0].tolist() == [1, 0]
    assert got[1][0].tolist() == [2.0 ** -11, 2.0 ** -11 + 2.0 ** -24]  # fused: [0, 1] with two equal scores


def test_by_hand_zeros_infinities_and_a_dropped_entry():
    """w = (0, 1): the distance does not count -- but 0 * inf is NaN, so the entry with d = +inf is dropped
         id 0: a -0.0 -> 0 * 2 + (1 * -0.0) = +0 + -0 = +0
         id 1: a  0.0 -> +0                          (ties with id 0 at +0: the id decides, +0 bits come back)
         id 2: a -3   -> -3
         id 3: a  5, d +inf -> NaN: never returned
       then w = (-1, 0): s = -d + 0 * a: d = +inf scores -inf and ranks FIRST; d = 0 scores -0 + 0 = +0"""
    table = np.array([[-0.0], [0.0], [-3], [5]], dtype=np.float32)
    ids = np.array([[1, 3, 0, 2]], dtype=np.uint32)
    dists = np.array([[2, np.inf, 2, 2]], dtype=np.float32)
    got = both(ids, dists, None, None, table, np.array([0, 1], dtype=np.float32), 4)
    assert got[0][0].tolist() == [2, 0, 1, MAX] and got[3][0] == 3 and got[4][0] == 0
    assert got[1][0].view(np.uint32).tolist() == [0xC0400000, 0, 0, 0x7F800000]
    dists = np.array([[2, np.inf, 0, 1]], dtype=np.float32)
    got = both(ids, dists, None, None, table, np.array([-1, 0], dtype=np.float32), 4)
    assert got[0][0].tolist() == [3, 1, 2, 0] and got[1][0].tolist() == [-np.inf, -2, -1, 0]
    assert got[1][0].view(np.uint32)[3] == 0 and got[2][0].tolist() == [np.inf, 2, 1, 0]


def test_boost_lists_refuses_shapes_beyond_the_limits():
    table = np.zeros((10, 4), dtype=np.float32)
    ids, dists, w = np.zeros((2, 8), dtype=np.uint32), np.zeros((2, 8), dtype=np.float32), np.zeros(5, dtype=np.float32)
    for a in ((ids, dists, None, None, table, w, 0), (ids, dists, None, None, table, w, 9),
              (ids, dists[:, :7], None, None, table, w, 1), (ids, dists, None, None, table, w[:4], 1),
              (ids, dists, None, None, table, np.zeros((3, 5), dtype=np.float32), 1),
              (ids, dists, None, None, table.astype(np.float64), w, 1),
              (np.zeros((2, 1025), dtype=np.uint32), np.zeros((2, 1025), dtype=np.float32), None, None, table, w, 1),
              (ids, dists, None, None, np.zeros((3, 33), dtype=np.float32), np.zeros(34, dtype=np.float32), 1)):
        with pytest.raises(ValueError):
            H.boost_lists(*a)
    got = H.boost_lists(np.zeros((2, 1024), dtype=np.uint32), np.zeros((2, 1024), dtype=np.float32), None, None,
                        np.zeros((3, 32), dtype=np.float32), np.zeros((2, 33), dtype=np.float32), 1024)
    assert got[3].tolist() == [1024, 1024]


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(nq=6, pool=16, n_out=10, n_attrs=8, dtype=0, table=fake, rows=100, w=fake, w_rows=1, i_in=fake, d_in=fake,
             c_in=fake, s_in=fake, ids=fake, scores=fake, dists=fake, counts=fake, stats=fake):
        return L.hnsw_boost_device(nq, pool, n_out, n_attrs, dtype, table, rows, w, w_rows, i_in, d_in, c_in, s_in, ids, scores,
                                   dists, counts, stats, None)

    for kw in (dict(pool=0), dict(n_out=0), dict(n_out=17), dict(pool=1025, n_out=1), dict(pool=0x80000000, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"boost: needs 1 <= n_out <= pool <= 1024", kw
    for kw in (dict(n_attrs=0), dict(n_attrs=33)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"boost: needs 1 <= n_attrs <= 32", kw
    for dtype in (2, 7, 0xFFFFFFFF):
        assert call(dtype=dtype) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"boost: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)"
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boost: at most 2^31 - 1 queries"
    for w_rows in (0, 2, 5, 7):
        assert call(w_rows=w_rows) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"boost: weights_rows is 1 (one row for every query) or nq"
    for name in ("table", "w", "i_in", "d_in", "ids", "scores"):
        assert call(pool=1024, n_out=1024, n_attrs=32, dtype=1, w_rows=6, **{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == \
            b"boost: needs the table, the weights, the candidates' ids and distances and the id and score outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boost: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # the order of the checks: the shape, nq, the weight rows, the pointers, the stats pair
    assert call(pool=0, nq=1 << 31, w_rows=3, table=None, stats=None) == _lib.ERR_ARG and b"n_out <= pool" in L.hnsw_last_error()
    assert call(nq=1 << 31, w_rows=3, table=None, stats=None) == _lib.ERR_ARG and b"2^31 - 1" in L.hnsw_last_error()
    assert call(w_rows=3, table=None, stats=None) == _lib.ERR_ARG and b"weights_rows" in L.hnsw_last_error()
    assert call(table=None, stats=None) == _lib.ERR_ARG and b"needs the table" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, pool=0, n_out=0, n_attrs=0, dtype=9, table=None, w=None, w_rows=0, i_in=None, d_in=None, ids=None,
                scores=None, stats=None) == _lib.OK
    with pytest.raises(H.HnswError) as e:
        H.boost_device(4, 10, 11, 8, "f32", 256, 100, 256, 1, 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        H.boost_device(4, 10, 5, 8, "bf16", 256, 100, 256, 1, 256, 256, None, None, 256, 256)
    H.HNSW.boost_device(0, 10, 5, 8, "f16", None, 0, None, 1, None, None, None, None, None, None)  # nq == 0


def test_search_argument_errors_need_no_device():
    index = small()
    other = small(n=50)
    A = 5
    tab, foreign, wide = index.row_table(A, "f16"), other.row_table(A, "f16"), index.row_table(33, "f32")
    Q, W = rand_vectors(6, D, 12), np.ones((6, 1 + A), dtype=np.float32)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    lo, hi = np.zeros(6, dtype=np.uint32), np.full(6, 5, dtype=np.uint32)

    def rc(h=index, t=tab, Q=Q, nq=6, n=4, pool=20, ef=32, w=W, w_rows=6, s=None, mask_of=None, lo=None, hi=None, ids="own"):
        o_i = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_s, o_d = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full((6, max(n, 1)), 2.5, dtype=np.float32)
        o_c = np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_boosted(None if h is None else h._h, None if t is None else t._t, ptr(Q, f32p), nq, n, pool,
                                           ef, ptr(w, f32p), w_rows, s, ptr(mask_of, u32p), ptr(lo, u32p), ptr(hi, u32p),
                                           ptr(o_i, u32p), ptr(o_s, f32p), ptr(o_d, f32p), ptr(o_c, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_s == 3.5).all() and (o_d == 2.5).all() and (o_c == 9).all() and (o_i is None or (o_i == 7).all())
        return code

    assert rc(h=None) == _lib.ERR_ARG
    assert rc(lo=lo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: a label range needs lo and hi, both or neither"
    assert rc(mask_of=lo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: mask_of needs its mask set"
    assert rc(t=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: needs a row table"
    assert rc(t=foreign) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: the row table belongs to another handle"
    for kw in (dict(pool=0), dict(n=0), dict(n=21), dict(pool=1025)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"boosted search: needs 1 <= n <= pool <= 1024", kw
    assert rc(t=wide, w=np.ones((6, 34), dtype=np.float32)) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: needs 1 <= the table's full_dim <= 32"
    assert rc(pool=65, lo=lo, hi=hi) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: needs pool <= 64 under a filter or while ids are deleted"
    for kw in (dict(Q=None), dict(w=None), dict(ids=None), dict(nq=1 << 31)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"boosted search: needs the queries, the weights, an id buffer and at most 2^31 - 1 queries", kw
    for w_rows in (0, 2, 7):
        assert rc(w_rows=w_rows) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"boosted search: weights_rows is 1 (one row for every query) or nq"
    assert rc() == _lib.ERR_ARG  # the table is empty: it does not cover the index
    assert L.hnsw_last_error() == b"boosted search: the row table has 0 rows, the index 300"
    assert rc(w_rows=1) == _lib.ERR_ARG and b"has 0 rows" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle and the filter's own refusals)
    assert rc(nq=0) == _lib.OK and rc(nq=0, t=None, Q=None, w=None, w_rows=0, ids=None, pool=0, n=0) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    # the candidate call's limit while ids are deleted
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65, n=4) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"boosted search: needs pool <= 64 under a filter or while ids are deleted"
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty, t=empty.row_table(A)) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    tab = index.row_table(4, "f32")
    Q, W = rand_vectors(6, D, 12), np.ones(5, dtype=np.float32)
    for bad_q, bad_w in ((Q[:, :5], W), (Q, W[:4]), (Q, np.ones((6, 4), dtype=np.float32)), (Q, np.ones((2, 3, 5), dtype=np.float32))):
        with pytest.raises(H.HnswError) as e:
            index.search_batch_boosted(tab, bad_q, bad_w, 3, 10, 32)
        assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_boosted(tab, Q, W, 3, 10, 32, lo=1)
    with pytest.raises(H.HnswError) as e:  # the library's own refusals, before any device
        index.search_batch_boosted(tab, Q, W, 11, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_boosted(tab, Q, np.ones((3, 5), dtype=np.float32), 3, 10, 32)
    assert e.value.code == _lib.ERR_ARG and "weights_rows" in str(e.value)
    got = index.search_batch_boosted(tab, Q[:0], W, 3, 10, 32)  # nq == 0
    assert got[0].shape == got[1].shape == got[2].shape == (0, 3) and got[3].shape == (0,) and got[4].shape == (0, 4)
    assert index.stat("uploads") == 0


# ---- the table's file ------------------------------------------------------------------------------------------------------
def header(magic=0x48585254, version=1, full_dim=3, dtype=0, rows=0):
    return struct.pack(">IIIIQ", magic, version, full_dim, dtype, rows)


def test_save_and_load_argument_errors_need_no_device(tmp_path):
    index = small(n=50)
    tab = index.row_table(3, "f32")
    L = _lib.lib()
    path = str(tmp_path / "t.hxrt").encode()
    t = C.c_void_p()
    assert L.hnsw_row_table_save(None, path) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"row table: saving needs a table and a path"
    assert L.hnsw_row_table_save(tab._t, None) == _lib.ERR_ARG
    assert L.hnsw_row_table_save(tab._t, str(tmp_path / "no" / "such" / "dir").encode()) == _lib.ERR_IO
    assert L.hnsw_last_error().startswith(b"row table: could not create ")
    for args in ((None, path, C.byref(t)), (index._h, None, C.byref(t)), (index._h, path, None)):
        assert L.hnsw_row_table_load(*args) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"row table: loading needs a handle, a path and a place for the table"
    assert L.hnsw_row_table_load(index._h, path, C.byref(t)) == _lib.ERR_IO  # no such file
    assert L.hnsw_last_error().startswith(b"row table: could not open ") and not t.value
    assert index.stat("row_table_writes") == 0 and index.stat("uploads") == 0


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_an_empty_table_round_trips_without_a_device(tmp_path, dtype):
    index = small(n=50)
    tab = index.row_table(7, dtype)
    path = tmp_path / "empty.hxrt"
    tab.save(path)
    assert open(path, "rb").read() == header(full_dim=7, dtype=tab.dtype, rows=0)  # the whole file: 24 bytes, big-endian
    back = index.load_row_table(path)
    assert (back.full_dim, back.dtype, back.rows) == (7, tab.dtype, 0) and back.device() == (None, 0)
    assert back._index is index and index.stat("row_table_writes") == 0 and index.stat("uploads") == 0
    back.close()


def test_corrupt_files_are_io_errors_before_any_device(tmp_path):
    index = small(n=50)
    L = _lib.lib()
    row = struct.pack(">3f", 1.0, -0.0, 2.5)
    cases = {
        "empty": (b"", b"shorter than its header"),
        "short header": (header()[:23], b"shorter than its header"),
        "magic": (header(magic=0x48585255), b"not a row table (magic)"),
        "little-endian magic": (struct.pack("<IIIIQ", 0x48585254, 1, 3, 0, 0), b"not a row table (magic)"),
        "version 0": (header(version=0), b"a version this library does not read"),
        "version 2": (header(version=2), b"a version this library does not read"),
        "full_dim 0": (header(full_dim=0), b"full_dim out of range"),
        "full_dim 4097": (header(full_dim=4097), b"full_dim out of range"),
        "dtype 2": (header(dtype=2), b"an unknown dtype"),
        "too many rows": (header(rows=1 << 32), b"more than 2^32 - 1 rows"),
        "a row missing": (header(rows=2) + row, b"its length is not what its header says"),
        "a byte missing": (header(rows=1) + row[:-1], b"its length is not what its header says"),
        "a byte too many": (header(rows=1) + row + b"\0", b"its length is not what its header says"),
        "rows behind an empty table": (header(rows=0) + row, b"its length is not what its header says"),
        "f16 length for f32": (header(rows=1) + row[:6], b"its length is not what its header says"),
        "a huge count": (header(rows=(1 << 32) - 1) + row, b"its length is not what its header says"),
        # (the elements are looked at chunk by chunk, before the chunk goes to a device: the first chunk here)
        "a NaN": (header(rows=1) + struct.pack(">3f", 1.0, float("nan"), 2.5), b"holds a NaN or an infinity"),
        "an infinity": (header(rows=2) + row + struct.pack(">3f", 1.0, 0.0, float("-inf")), b"holds a NaN or an infinity"),
        "an f16 infinity": (header(dtype=1, rows=1) + struct.pack(">3H", 0x3C00, 0x7C00, 0), b"holds a NaN or an infinity"),
        "an f16 NaN": (header(dtype=1, rows=1) + struct.pack(">3H", 0x3C00, 0xFE01, 0), b"holds a NaN or an infinity"),
    }
    for name, (blob, why) in cases.items():
        path = tmp_path / "bad.hxrt"
        path.write_bytes(blob)
        t = C.c_void_p()
        assert L.hnsw_row_table_load(index._h, str(path).encode(), C.byref(t)) == _lib.ERR_IO, name
        assert L.hnsw_last_error().endswith(b": " + why), (name, L.hnsw_last_error())
        assert not t.value, name
        with pytest.raises(H.HnswError) as e:
            index.load_row_table(path)
        assert e.value.code == _lib.ERR_IO, name
    assert index.stat("row_table_writes") == 0 and index.stat("uploads") == 0


# ---- the kernel that carries the new form ------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernel_carries_the_boost_without_scratch_spills_or_lost_occupancy(tmp_path):
    """exact_scan.hip compiled for gfx950 with the Makefile's flags: the boost is a source form of hx_distance_kernel,
    selected by a field of its own that launch_boost alone sets and looked at before every other form; the kernel's two
    instantiations stay the only ones, and run without scratch, without spilled vector registers and at the occupancy
    they had before the form"""
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "exact_scan.hip")
    text = open(src).read()
    assert "boost_lists(dv, smem, lane)" in text, "the boost is a source form of hx_distance_kernel"
    assert text.index("if (dv.boost)") < text.index("if (dv.hybrid)"), "looked at before every other form"
    assert len(re.findall(r"\bd\.boost = ", text)) == 1 and "d.boost = 1 + d.mode" in text, "one launcher sets the selector"
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
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r.get("VGPRs", 0) <= 256 and r["Occupancy"] == 1, (name, r)  # (one wave per SIMD: as before the form)
