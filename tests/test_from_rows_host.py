"""Search from stored rows on the host (include/hnsw_mi355x.h, "search from stored rows"): the numpy restatements of the
fold and of the drop (hnsw_rs_amd.from_rows.compose_rows, drop_ids) against second, deliberately plain ones
(tests/from_rows_cases.py) bit for bit, the row of an id against hnsw_get_vector and the oracle, and everything the four
entry points decide before they touch a device -- every argument error with its message, nq == 0, the stat keys, the
exported symbols and their prototypes.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import from_rows_cases as FC
from tests.util import oracle_from_product, rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
NEW_SYMBOLS = ("hnsw_compose_rows_device", "hnsw_drop_ids_device", "hnsw_search_batch_from_rows", "hnsw_search_batch_by_id")
KEYS = ("uploads", "from_rows_calls", "from_rows_compose_launches", "from_rows_drop_launches")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the fold against the plain loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", FC.WIDTHS)
def test_compose_rows_is_the_plain_loop_bit_for_bit(width):
    n, d = 300, 9
    rows = (rand_vectors(n, d, 3) - np.float32(0.5)).astype(np.float32)
    rows[11, 2], rows[11, 5] = -0.0, 0.0
    asked = []

    def get_row(i):
        asked.append(i)
        return rows[i]

    src, w = FC.compose_slots(width, n, 40 + width)
    for weights in (w, None):
        got = H.compose_rows(src, weights, get_row, n)
        want = FC.naive_compose(src, weights, lambda i: rows[i], n, d)
        assert np.array_equal(got[1], want[1]), (width, got[1], want[1])
        assert np.array_equal(bits(got[0]), bits(want[0])), "width %d weights %s" % (width, weights is not None)
        assert got[0].shape == (src.shape[0], d) and got[0].dtype == np.float32
        # a query of pads only and an id equal to the length: ERR_ARG, a row of zeros, no row asked for
        assert got[1][4] == _lib.ERR_ARG and got[1][5] == _lib.ERR_ARG
        assert (bits(got[0][4]) == 0).all() and (bits(got[0][5]) == 0).all()
        assert n not in asked and (got[1][[0, 1, 2, 3, 6, 7]] == 0).all()
    # weights None against explicit ones give the same bits
    ones = H.compose_rows(src, np.ones(src.shape, dtype=np.float32), get_row, n)
    none = H.compose_rows(src, None, get_row, n)
    assert np.array_equal(bits(ones[0]), bits(none[0])) and np.array_equal(ones[1], none[1])
    # +inf and NaN weights reach the row
    got = H.compose_rows(src, w, get_row, n)
    assert np.isnan(got[0][9]).any() and got[1][9] == 0
    assert not np.isfinite(got[0][8]).all() and got[1][8] == 0
    if width == 1:  # one slot, no weights: the row itself, a -0.0 element stays -0.0
        assert np.array_equal(bits(none[0][6]), bits(rows[11])) and bits(none[0][6])[2] == 0x80000000


def test_compose_rows_refuses_bad_shapes():
    get_row = lambda i: np.zeros(4, dtype=np.float32)  # noqa: E731
    with pytest.raises(ValueError):
        H.compose_rows(np.zeros((2, 65), dtype=np.uint32), None, get_row, 10)
    with pytest.raises(ValueError):
        H.compose_rows(np.zeros((2, 0), dtype=np.uint32), None, get_row, 10)
    with pytest.raises(ValueError):
        H.compose_rows(np.zeros((2, 3), dtype=np.uint32), np.zeros((2, 2), dtype=np.float32), get_row, 10)
    with pytest.raises(ValueError):  # no query can be composed and the dimension is not given
        H.compose_rows(np.full((2, 3), MAX, dtype=np.uint32), None, get_row, 10)
    got = H.compose_rows(np.full((2, 3), MAX, dtype=np.uint32), None, get_row, 10, dim=4)
    assert got[0].shape == (2, 4) and (got[1] == _lib.ERR_ARG).all()
    got = H.compose_rows(np.array([3, 4], dtype=np.uint32), None, get_row, 10)  # [nq]: one slot each
    assert got[0].shape == (2, 4) and (got[1] == 0).all()


@pytest.mark.parametrize("kind,d", [(H.VEC_F32, 16), (H.VEC_QUANT8, 23)], ids=["f32-16", "quant8-23"])
def test_one_slot_without_weights_is_get_vector_and_the_oracles_row(kind, d):
    n = 400
    vs = rand_vectors(n, d, 7)
    lv = O.draw_levels(n, 8, 7)
    index = H.HNSW.new(8, 32, d, kind).insert_bulk(vs, 2, False, levels=lv)
    orc = oracle_from_product(index, vs, lv)
    src = np.arange(0, n, 7, dtype=np.uint32).reshape(-1, 1)
    L = _lib.lib()
    direct = np.zeros((src.shape[0], d), dtype=np.float32)
    for k, i in enumerate(src[:, 0].tolist()):
        assert L.hnsw_get_vector(index._h, i, ptr(direct[k], f32p)) == _lib.OK
    got = H.compose_rows(src, None, lambda i: index.get_point(i).get_vals(), n)
    assert (got[1] == 0).all() and np.array_equal(bits(got[0]), bits(direct))
    got = H.compose_rows(src, None, orc.get_vals, n)
    assert np.array_equal(bits(got[0]), bits(direct))


# ---- the drop against the plain loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,width", FC.drop_sweep())
def test_drop_ids_is_the_plain_loop(n_in, width):
    seen_drop = seen_twice = False
    for with_counts in (True, False):
        ids, dists, counts, statuses, ex, src_st = FC.drop_lists(n_in, width, with_counts, seed=1000 * n_in + 10 * width + with_counts)
        for n_out in FC.n_outs(n_in):
            for src in (None, src_st):
                what = "n_in=%d width=%d counts=%s n_out=%d src=%s" % (n_in, width, with_counts, n_out, src is not None)
                got = H.drop_ids(ids, dists, counts, statuses, ex, n_out, src)
                want = FC.naive_drop(ids, dists, counts, statuses, ex, n_out, src)
                FC.assert_drop_equal(got, want, what)
                assert np.array_equal(got[4], want[4]), what
                assert got[0].shape == got[1].shape == (FC.NQ, n_out) and got[2].shape == got[3].shape == (FC.NQ,)
                # the planted queries did what they are there for
                assert got[3][0] == 1 and got[3][1] == 1 and got[3][2] == 1 and got[3][3] == 0, (what, got[3])
                assert got[2][6] == 0 and got[4][6] == FC.ERR_NAN_INPUT and (got[0][6] == MAX).all() and got[3][6] == 0
                assert got[2][7] == 0 and got[3][7] == min(width, n_in), what
                assert got[2][9] == 0 and got[3][9] == 0
                assert got[3][10] == 1
                if src is not None:
                    assert got[2][11] == 0 and got[4][11] == FC.ERR_ARG and got[3][11] == 0
                else:
                    assert got[4][11] == 0 and got[3][11] == 1
                if n_in >= 3:
                    assert got[3][4] == 2, what  # an entry listed twice counts twice
                    seen_twice = True
                if width >= 2:
                    assert got[3][5] == (2 if width >= 3 and n_in >= 2 else 1), what  # an exclusion id given twice: one entry
                    assert got[3][8] == 1, what  # pads in the exclusion list never match the pads among the entries
                else:
                    assert got[3][8] == 0
                pads = got[0] == MAX
                assert np.isposinf(got[1][pads]).all() and (np.arange(n_out)[None, :] >= got[2][:, None])[pads].all()
                seen_drop = True
    assert seen_drop and (seen_twice or n_in < 3)


def test_drop_ids_refuses_shapes_beyond_the_limits():
    ids, dists = np.zeros((2, 1100), dtype=np.uint32), np.zeros((2, 1100), dtype=np.float32)
    ex = np.zeros((2, 3), dtype=np.uint32)
    for a in ((ids, dists, None, None, ex, 1), (ids[:, :10], dists[:, :10], None, None, ex, 11),
              (ids[:, :10], dists[:, :10], None, None, ex, 0), (ids[:, :10], dists[:, :9], None, None, ex, 1),
              (ids[:, :10], dists[:, :10], None, None, np.zeros((2, 65), dtype=np.uint32), 1),
              (ids[:, :10], dists[:, :10], None, None, np.zeros((3, 2), dtype=np.uint32), 1)):
        with pytest.raises(ValueError):
            H.drop_ids(*a)


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_compose_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, width=3, src=fake, w=fake, Q=fake, st=fake):
        return L.hnsw_compose_rows_device(h, nq, width, src, w, Q, st, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for width in (0, 65, 1 << 20):
        assert call(width=width) == _lib.ERR_ARG, width
        assert L.hnsw_last_error() == b"compose rows: needs 1 <= width <= 64", width
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"compose rows: at most 2^31 - 1 queries"
    for name in ("src", "Q"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == b"compose rows: needs the source ids and the query rows", name
    assert call(nq=0) == _lib.OK and call(nq=0, width=0, src=None, Q=None, w=None, st=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0


def test_drop_argument_errors_need_no_device():
    L = _lib.lib()
    fake = C.c_void_p(256)

    def call(nq=6, n_in=20, n_out=10, width=3, ex=fake, src_st=fake, i_in=fake, d_in=fake, c_in=fake, s_in=fake, ids=fake,
             dists=fake, counts=fake, dropped=fake, stats=fake):
        return L.hnsw_drop_ids_device(nq, n_in, n_out, width, ex, src_st, i_in, d_in, c_in, s_in, ids, dists, counts, dropped,
                                      stats, None)

    for kw in (dict(n_out=0), dict(n_in=0, n_out=0), dict(n_out=21), dict(n_in=1025, n_out=10), dict(n_in=1025, n_out=1025)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"drop ids: needs 1 <= n_out <= n_in <= 1024", kw
    for width in (0, 65):
        assert call(width=width) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"drop ids: needs 1 <= width <= 64"
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"drop ids: at most 2^31 - 1 queries"
    for name in ("ex", "i_in", "d_in", "ids", "dists"):
        assert call(n_in=1024, n_out=1024, width=64, **{name: None}) == _lib.ERR_ARG, name  # (within the limits)
        assert L.hnsw_last_error() == (b"drop ids: needs the exclusion ids, the candidates' ids and distances and the id and "
                                       b"distance outputs"), name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"drop ids: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    assert call(nq=0) == _lib.OK
    assert call(nq=0, n_in=0, n_out=0, width=0, ex=None, i_in=None, d_in=None, ids=None, dists=None, stats=None) == _lib.OK


def test_search_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    good = (np.arange(18, dtype=np.uint32) * 5).reshape(6, 3)

    def rc(h=index, src=good, w=None, nq=6, width=3, n=4, ef=32, exclude=1, ids="own", by_id=False):
        o_ids = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_d, o_c = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full(6, 9, dtype=np.uint32)
        hh = None if h is None else h._h
        if by_id:
            code = L.hnsw_search_batch_by_id(hh, ptr(src, u32p), nq, n, ef, exclude, ptr(o_ids, u32p), ptr(o_d, f32p),
                                             ptr(o_c, u32p), None)
        else:
            code = L.hnsw_search_batch_from_rows(hh, ptr(src, u32p), ptr(w, f32p), nq, width, n, ef, exclude, ptr(o_ids, u32p),
                                                 ptr(o_d, f32p), ptr(o_c, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_d == 3.5).all() and (o_c == 9).all() and (o_ids is None or (o_ids == 7).all())
        return code

    for by_id in (False, True):
        assert rc(h=None, by_id=by_id) == _lib.ERR_ARG
        assert b"null handle" in L.hnsw_last_error()
        assert rc(n=0, by_id=by_id) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"search from rows: needs n >= 1 and n + width <= 1024"
        assert rc(src=None, by_id=by_id) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"search from rows: needs source ids, an id buffer and at most 2^31 - 1 queries"
        assert rc(ids=None, by_id=by_id) == _lib.ERR_ARG
        assert rc(nq=1 << 31, by_id=by_id) == _lib.ERR_ARG
        assert rc(ef=(1 << 26) + 1, by_id=by_id) == _lib.ERR_ARG
    for width in (0, 65):
        assert rc(width=width) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"search from rows: needs 1 <= width <= 64"
    assert rc(n=1022) == _lib.ERR_ARG  # n + width = 1025
    assert L.hnsw_last_error() == b"search from rows: needs n >= 1 and n + width <= 1024"
    assert rc(n=1022, exclude=0) == _lib.ERR_ARG  # (the limit does not depend on the drop)
    assert rc(n=1024, by_id=True) == _lib.ERR_ARG
    # a source id out of range, or a query without a source, fails the whole call and names its query
    bad = good.copy()
    bad[4, 1] = N
    assert rc(src=bad) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"search from rows: query 4 names source id 700, the index has 700 points"
    bad = good.copy()
    bad[2, :] = MAX
    assert rc(src=bad) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"search from rows: query 2 has no source"
    one = np.arange(6, dtype=np.uint32)
    one[5] = N + 3
    assert rc(src=one, by_id=True) == _lib.ERR_ARG
    assert b"query 5 names source id 703" in L.hnsw_last_error()
    one[5] = MAX
    assert rc(src=one, by_id=True) == _lib.ERR_ARG
    assert b"query 5 has no source" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle)
    assert rc(nq=0) == _lib.OK and rc(nq=0, src=None, ids=None, width=0, n=0) == _lib.OK and rc(nq=0, by_id=True) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    index.mark_deleted(np.array([3, 5]))
    assert rc(n=62) == _lib.ERR_ARG  # n + width = 65 while ids are deleted
    assert L.hnsw_last_error() == b"search from rows: needs n + width <= 64 while ids are deleted"
    assert rc(n=62, exclude=0) == _lib.ERR_ARG
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY and rc(h=empty, by_id=True) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    with pytest.raises(ValueError):
        index.search_batch_from_rows(np.arange(6, dtype=np.uint32), None, 3, 32)  # [nq, width] wanted
    with pytest.raises(ValueError):
        index.search_batch_from_rows(np.zeros((2, 3), dtype=np.uint32), np.ones((2, 2), dtype=np.float32), 3, 32)
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_from_rows(np.zeros((2, 65), dtype=np.uint32), None, 3, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_by_id([1, 2, N], 3, 32)
    assert e.value.code == _lib.ERR_ARG and "query 2" in str(e.value)
    with pytest.raises(H.HnswError) as e:
        index.knn_graph(3, 32, chunk=100, ids=[5, N + 1])
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_from_rows(np.zeros((0, 3), dtype=np.uint32), None, 3, 32)  # nq == 0
    assert got[0].shape == got[1].shape == (0, 3) and got[2].shape == (0,)
    got = index.search_batch_by_id([], 3, 32)
    assert got[0].shape == (0, 3)
    got = index.knn_graph(3, 32, ids=[])
    assert got[0].shape == got[1].shape == (0, 3) and got[2].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.compose_rows_device(4, 65, 256, None, 256)
    assert e.value.code == _lib.ERR_ARG
    index.compose_rows_device(0, 3, None, None, None)  # nq == 0
    with pytest.raises(H.HnswError) as e:
        H.HNSW.drop_ids_device(4, 10, 11, 1, 256, None, 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    H.HNSW.drop_ids_device(0, 10, 3, 1, None, None, None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("from_rows_calls", "from_rows_compose_launches", "from_rows_drop_launches"):
        assert index.stat(key) == 0


def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers d_*, the stream and the handle
    are bound as void pointers)"""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind in ("void*", "hnsw_index*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "float": C.c_float, "int": C.c_int, "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int
        assert [c_type_of(p) for p in params] == argtypes, name
    assert [len(_lib.SYMBOLS[s][1]) for s in NEW_SYMBOLS] == [8, 16, 12, 10]
    assert re.search(r"#define HNSW_FROM_ROWS_MAX_TERMS 64\b", header) and H.FROM_ROWS_MAX_TERMS == 64
    assert re.search(r"#define HNSW_DROP_MAX_N 1024\b", header) and H.DROP_MAX_N == 1024 == H.RADIUS_MAX_N
    for method in ("search_batch_from_rows", "search_batch_by_id", "knn_graph", "compose_rows_device", "drop_ids_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.compose_rows) and callable(H.drop_ids)
