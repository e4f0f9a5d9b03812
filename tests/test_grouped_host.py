"""Grouped search on the host (include/hnsw_mi355x.h, "grouped search"): the numpy restatement of the collapse
(hnsw_rs_amd.grouped.group_by_label) against a second, deliberately naive one (tests/grouped_cases.py) bit for bit, and
everything hnsw_group_by_label_device and hnsw_search_batch_grouped decide before they touch a device -- every argument
error with its message, nq == 0, the stat keys, the exported symbols and their prototypes.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import grouped_cases as GC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_group_by_label_device", "hnsw_search_batch_grouped")
KEYS = ("uploads", "label_words_uploaded", "grouped_calls", "grouped_launches", "filtered_range_calls", "filtered_set_calls",
        "filtered_set_range_calls", "filtered_queries_graph", "filtered_queries_exact")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the naive one ----------------------------------------------------------------------------
@pytest.mark.parametrize("pool", GC.POOLS)
def test_group_by_label_is_the_naive_collapse_bit_for_bit(pool):
    labels = GC.column()
    seen_overflow = seen_short = False
    for with_counts in (True, False):
        ids, dists, counts = GC.synthetic_lists(pool, with_counts, seed=100 * pool + with_counts)
        for G, P in GC.shapes(pool):
            what = "pool=%d counts=%s G=%d P=%d" % (pool, with_counts, G, P)
            got = H.group_by_label(ids, dists, counts, labels, G, P)
            want = GC.naive(ids, dists, counts, labels, G, P)
            GC.assert_grouped_equal(got, want, what)
            assert got[0].shape == (GC.NQ, G, P) and got[2].shape == (GC.NQ, G) and got[4].shape == (GC.NQ,)
            # the planted queries did what they are there for
            assert got[4][0] == 0 and (got[0][0] == MAX).all() and np.isposinf(got[1][0]).all() and (got[3][0] == 0).all()
            assert got[4][1] == 1 and got[2][1, 0] == 77 and got[3][1, 0] == min(P, pool)
            assert got[4][2] == min(G, pool) and (got[3][2, :got[4][2]] == 1).all()
            assert got[4][4] == 1 and got[2][4, 0] == 0 and (got[0][4, 0, :min(P, pool)] >= GC.N_LABELS).all()
            assert set(got[2][3, :got[4][3]].tolist()) <= {0, 1, 2, 3, MAX}
            seen_overflow |= bool((got[3] == P).any() and P < pool)
            seen_short |= bool((got[4] < G).any())
        # a handle without labels: one group of label 0
        got = H.group_by_label(ids, dists, counts, None, 1, pool)
        GC.assert_grouped_equal(got, GC.naive(ids, dists, counts, None, 1, pool), "no labels, pool=%d" % pool)
        assert (got[2] == 0).all() and (got[4] <= 1).all()
    assert seen_short and (seen_overflow or pool == 1)


def test_group_by_label_refuses_shapes_beyond_the_limits():
    ids, dists = np.zeros((2, 300), dtype=np.uint32), np.zeros((2, 300), dtype=np.float32)
    for a in ((ids, dists, None, None, 1, 1), (ids[:, :10], dists[:, :10], None, None, 11, 1),
              (ids[:, :10], dists[:, :10], None, None, 1, 11), (ids[:, :10], dists[:, :10], None, None, 0, 1),
              (ids[:, :64], dists[:, :64], None, None, 33, 32), (ids[:, :10], dists[:, :9], None, None, 1, 1)):
        with pytest.raises(ValueError):
            H.group_by_label(*a)


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, pool=64, G=4, P=3, i_in=fake, d_in=fake, c_in=fake, s_in=fake, ids=fake, dists=fake,
             labels=fake, sizes=fake, counts=fake, stats=fake):
        return L.hnsw_group_by_label_device(h, nq, pool, G, P, i_in, d_in, c_in, s_in, ids, dists, labels, sizes, counts,
                                            stats, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(pool=0), dict(pool=257), dict(G=0), dict(P=0), dict(G=65), dict(P=65), dict(pool=256, G=33, P=32),
               dict(pool=256, G=256, P=5)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"n_groups x per_group <= 1024" in L.hnsw_last_error(), kw
    assert call(pool=256, G=32, P=32, i_in=None) == _lib.ERR_ARG  # (1024 slots are within the limits: the pointer is refused)
    assert b"needs the candidates" in L.hnsw_last_error()
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert b"2^31 - 1" in L.hnsw_last_error()
    for name in ("i_in", "d_in", "ids", "dists", "labels", "sizes"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert b"needs the candidates" in L.hnsw_last_error(), name
    assert call(s_in=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    assert call(stats=None) == _lib.ERR_ARG
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, pool=0, G=0, P=0, i_in=None, d_in=None, ids=None, dists=None, labels=None, sizes=None, stats=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before


def test_search_argument_errors_need_no_device():
    index, other = small(), small(seed=2)
    index.set_labels(np.arange(N, dtype=np.uint32) % 5)
    s, foreign = index.mask_set([np.ones(N, dtype=bool)]), other.mask_set([np.ones(N, dtype=bool)])
    Q = rand_vectors(6, D, 12)
    mo = np.zeros(6, dtype=np.uint32)
    lo, hi = np.zeros(6, dtype=np.uint32), np.full(6, 3, dtype=np.uint32)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h=index, Q=Q, nq=6, G=4, P=3, pool=20, ef=32, st=None, mo=None, lo=None, hi=None, ids="own", labels="own"):
        o_ids = np.full((6, max(G * P, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_lab = np.full((6, max(G, 1)), 7, dtype=np.uint32) if isinstance(labels, str) else labels
        o_d, o_sz, o_c = np.full((6, max(G * P, 1)), 3.5, dtype=np.float32), np.full((6, max(G, 1)), 9, dtype=np.uint32), \
            np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_grouped(None if h is None else h._h, ptr(Q, f32p), nq, G, P, pool, ef,
                                           None if st is None else st._s, ptr(mo, u32p), ptr(lo, u32p), ptr(hi, u32p),
                                           ptr(o_ids, u32p), ptr(o_d, f32p), ptr(o_lab, u32p), ptr(o_sz, u32p), ptr(o_c, u32p),
                                           None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_d == 3.5).all() and (o_sz == 9).all() and (o_c == 9).all()
            assert (o_ids is None or (o_ids == 7).all()) and (o_lab is None or (o_lab == 7).all())
        return code

    assert rc(h=None) == _lib.ERR_ARG
    for kw in (dict(pool=0), dict(pool=257), dict(G=0), dict(P=0), dict(G=21), dict(P=21), dict(pool=256, G=33, P=32)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert b"n_groups x per_group <= 1024" in L.hnsw_last_error(), kw
    assert rc(mo=mo) == _lib.ERR_ARG
    assert b"mask_of needs its mask set" in L.hnsw_last_error()
    assert rc(lo=lo) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    assert rc(hi=hi) == _lib.ERR_ARG
    assert rc(st=foreign) == _lib.ERR_ARG
    assert b"another handle" in L.hnsw_last_error()
    assert rc(Q=None) == _lib.ERR_ARG
    assert b"needs queries" in L.hnsw_last_error()
    assert rc(ids=None) == _lib.ERR_ARG and rc(labels=None) == _lib.ERR_ARG
    assert rc(nq=1 << 31) == _lib.ERR_ARG
    # the candidate call's limits: pool <= 64 under a filter or while ids are deleted ...
    for kw in (dict(st=s), dict(lo=lo, hi=hi), dict(st=s, mo=mo, lo=lo, hi=hi)):
        assert rc(pool=65, **kw) == _lib.ERR_ARG, kw
        assert b"pool <= 64" in L.hnsw_last_error()
    # ... and ef' <= 256 on the graph path, refused by the candidate call's planner, on the host
    index.set_option("filter_exact_max", -1)
    assert rc(lo=lo, hi=hi, ef=257) == _lib.ERR_ARG
    assert b"graph path" in L.hnsw_last_error()
    bad_row = mo.copy()
    bad_row[4] = 3
    assert rc(st=s, mo=bad_row) == _lib.ERR_ARG
    assert b"query 4 names mask" in L.hnsw_last_error()
    index.set_option("filter_exact_max", 65536)
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle and the filter's own consistency)
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, labels=None, pool=0, G=0, P=0) == _lib.OK
    assert rc(nq=0, st=foreign) == _lib.ERR_ARG and rc(nq=0, mo=mo) == _lib.ERR_ARG
    after = {k: index.stat(k) for k in KEYS}
    assert after == before
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65) == _lib.ERR_ARG
    assert b"pool <= 64" in L.hnsw_last_error()
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY
    for x in (s, foreign):
        x.close()


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(6, D, 12)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_grouped(Q[:, :5], 3, 2, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_grouped(Q, 3, 2, 10, 32, lo=1)
    with pytest.raises(ValueError):
        index.search_batch_grouped(Q, 3, 2, 10, 32, lo=[0, 1], hi=3)
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_grouped(Q, 11, 2, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_grouped(Q, 3, 2, 10, 32, mask_of=[0] * 6)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_grouped(Q[:0], 3, 2, 10, 32)  # nq == 0
    assert got[0].shape == (0, 3, 2) and got[2].shape == (0, 3) and got[4].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.group_by_label_device(4, 10, 11, 1, 256, 256, None, None, 256, 256, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.group_by_label_device(0, 10, 3, 2, None, None, None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("grouped_calls", "grouped_launches"):
        assert index.stat(key) == 0


def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers d_*, the stream, the handle and
    the set are bound as void pointers)"""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind in ("void*", "hnsw_index*", "hnsw_mask_set*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 16 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 17
    assert re.search(r"#define HNSW_GROUP_POOL_MAX 256\b", header) and H.GROUP_POOL_MAX == 256
    for method in ("search_batch_grouped", "group_by_label_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.group_by_label)
