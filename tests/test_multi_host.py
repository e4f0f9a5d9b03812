"""Multi-vector search on the host (include/hnsw_mi355x.h, "multi-vector search"): the numpy restatement of the fusion
(hnsw_rs_amd.multi.fuse_lists) against a second, deliberately plain one (tests/multi_cases.py) bit for bit, and
everything hnsw_fuse_lists_device and hnsw_search_batch_multi decide before they touch a device -- every argument error
with its message, nq == 0, the stat keys, the exported symbols and their prototypes.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import multi_cases as MC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_fuse_lists_device", "hnsw_search_batch_multi")
KEYS = ("uploads", "multi_calls", "multi_fuse_launches")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,pool", MC.SHAPES)
def test_fuse_lists_is_the_plain_loop_bit_for_bit(T, pool):
    dist = MC.table_dist()
    seen_short = False
    for with_counts in (True, False):
        Q, ids, counts, statuses = MC.synthetic(T, pool, with_counts, seed=1000 * T + 10 * pool + with_counts)
        for mode in (MC.SUM, MC.MIN):
            by_kind = {}
            for kind in MC.WEIGHT_KINDS:
                w = MC.weights_of(kind, T, seed=T + pool)
                for n_out in MC.n_outs(pool):
                    # the planted queries alone where the plain loop is longest (the same properties, less Python time)
                    k = MC.N_PLANTED if T * pool >= 200 and n_out == pool else MC.NQ
                    if kind == "mixed":
                        k = MC.NQ
                    cut = lambda a: None if a is None else a[:k]  # noqa: E731
                    what = "T=%d pool=%d counts=%s mode=%d weights=%s n_out=%d" % (T, pool, with_counts, mode, kind, n_out)
                    got = H.fuse_lists(cut(Q), cut(w), mode, cut(ids), cut(counts), cut(statuses), dist, n_out, MC.ID_SPAN)
                    want = MC.naive(cut(Q), cut(w), mode, cut(ids), cut(counts), cut(statuses), dist, n_out, MC.ID_SPAN)
                    MC.assert_fused_equal(got, want, what)
                    by_kind[(kind, n_out)] = got
                    assert got[0].shape == got[1].shape == (k, n_out) and got[2].shape == got[3].shape == (k,)
                    # the planted queries did what they are there for
                    assert got[2][0] == 0 and got[3][0] == 0 and got[4][0] == 0 and (got[0][0] == MAX).all()
                    assert got[3][1] == pool and got[3][2] == T * pool, what
                    assert got[3][3] <= T * pool - (2 if pool >= 3 else 0)
                    assert got[4][4] == (MC.ERR_NAN_INPUT if T > 1 else MC.ERR_OVERFLOW) and got[4][5] == MC.ERR_OVERFLOW
                    assert got[4][6] == MC.ERR_ARG and got[4][7] == MC.ERR_NAN_INPUT
                    for q in (4, 5, 6, 7):
                        assert got[2][q] == 0 and got[3][q] == 0 and (got[0][q] == MAX).all() and np.isposinf(got[1][q]).all()
                    assert got[4][8] == 0 and (got[3][8] >= 1 or pool < 4)
                    sel = got[0] != MAX
                    assert not np.isnan(got[1][sel]).any()  # a NaN score is never returned
                    assert (got[2] == sel.sum(axis=1)).all() and (got[2] <= got[3]).all()
                    for q in range(k):  # distinct ids, in (score, id) order
                        c = int(got[2][q])
                        assert len(set(got[0][q, :c].tolist())) == c
                        s, i = got[1][q, :c], got[0][q, :c].astype(np.int64)
                        assert all(s[a] < s[a + 1] or (s[a] == s[a + 1] and i[a] < i[a + 1]) for a in range(c - 1)), what
                    seen_short |= bool((got[2][got[4] == 0] < np.minimum(n_out, got[3][got[4] == 0])).any())
                    if kind == "mixed" and T == 1:  # a NaN weight is no error: under SUM every score is NaN and nothing is
                        assert got[4][11] == 0 and got[3][11] == want[3][11]  # returned, under MIN every score stays +inf
                        assert got[2][11] == 0 if mode == MC.SUM else np.isposinf(got[1][11, :got[2][11]]).all()
            for n_out in MC.n_outs(pool):  # no weights and weights of 1.0: the same bits
                a, b = by_kind[("none", n_out)], by_kind[("ones", n_out)]
                MC.assert_fused_equal(a[:4], tuple(x[:a[0].shape[0]] for x in b[:4]), "ones against none")
    assert seen_short or T * pool < 16  # (a NaN term, a NaN weight or inf - inf took candidates out somewhere)


def explicit_dist(table):
    return lambda q_row, ids: np.array([table[int(q_row[0])][int(i)] for i in ids], dtype=np.float32)


def test_equal_scores_go_to_the_lower_id_whatever_the_list_order():
    nan = float("nan")
    table = {0: {5: 1.0, 9: 0.5, 2: 1.0, 7: 0.25}, 1: {5: 0.5, 9: 1.0, 2: 0.5, 7: nan}}
    Q = np.array([[[0, 0], [1, 0]]], dtype=np.float32)
    for lists in ([[9, 5], [7, 2]], [[2, 7], [5, 9]], [[5, 5], [9, 2]]):
        ids = np.array([lists], dtype=np.uint32)
        for fn in (H.fuse_lists, MC.naive):
            got = fn(Q, None, MC.SUM, ids, None, None, explicit_dist(table), 2)
            full = len({x for l in lists for x in l})
            assert got[3][0] == full
            # 2, 5 and 9 all score 1.5; 7 scores NaN under SUM and is never returned
            assert got[0][0].tolist() == sorted(x for l in lists for x in l if x != 7)[:2] and (got[1][0] == 1.5).all()
            got = fn(Q, None, MC.MIN, ids, None, None, explicit_dist(table), 2)
            if 7 in lists[0] + lists[1]:  # under MIN the NaN term leaves the minimum as it is: 7 scores 0.25
                assert got[0][0, 0] == 7 and got[1][0, 0] == 0.25


def test_minus_zero_and_plus_zero_are_one_score():
    nan = float("nan")
    # under MIN with weights (-1, 1): id 8 scores -0.0 (its first term), id 3 scores +0.0 (its first term is NaN)
    table = {0: {8: 0.0, 3: nan, 4: 0.5}, 1: {8: 0.0, 3: 0.0, 4: 0.0}}
    Q = np.array([[[0, 0], [1, 0]]], dtype=np.float32)
    w = np.array([[-1.0, 1.0]], dtype=np.float32)
    ids = np.array([[[8, 4], [3, MAX]]], dtype=np.uint32)
    for fn in (H.fuse_lists, MC.naive):
        got = fn(Q, w, MC.MIN, ids, None, None, explicit_dist(table), 2)
        assert got[0][0].tolist() == [4, 3]  # -0.5, then the zeros by id: 3 before 8
        got = fn(Q, w, MC.MIN, ids, None, None, explicit_dist(table), 2, 100)
        assert got[3][0] == 3
        full = fn(Q, w, MC.MIN, np.array([[[8, 4, 3], [3, MAX, 8]]], dtype=np.uint32), None, None, explicit_dist(table), 3)
        assert full[0][0].tolist() == [4, 3, 8]
        assert full[1][0].view(np.uint32).tolist() == [0xBF000000, 0x00000000, 0x80000000]  # the fold's own bits


def test_fuse_lists_refuses_shapes_beyond_the_limits():
    dist = MC.table_dist()
    Q = np.zeros((2, 17, 2), dtype=np.float32)
    ids = np.zeros((2, 17, 4), dtype=np.uint32)
    for a in ((Q, None, "sum", ids, None, None, dist, 1), (Q[:, :4], None, "sum", ids[:, :4], None, None, dist, 5),
              (Q[:, :4], None, "sum", ids[:, :4], None, None, dist, 0), (Q[:, :3], None, "sum", ids[:, :4], None, None, dist, 1),
              (Q[:, :4], None, "max", ids[:, :4], None, None, dist, 1),
              (Q[:, :4], np.ones((2, 3), dtype=np.float32), "sum", ids[:, :4], None, None, dist, 1),
              (Q[:, :2], None, "sum", np.zeros((2, 2, 129), dtype=np.uint32), None, None, dist, 1)):
        with pytest.raises(ValueError):
            H.fuse_lists(*a)
    got = H.fuse_lists(Q[:, :4], None, "min", ids[:, :4], None, None, dist, 4)
    assert got[3].tolist() == [1, 1] and got[2].tolist() == [1, 1]


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, T=3, pool=16, n_out=10, mode=0, Q=fake, w=fake, i_in=fake, c_in=fake, s_in=fake, ids=fake,
             scores=fake, counts=fake, unique=fake, stats=fake):
        return L.hnsw_fuse_lists_device(h, nq, T, pool, n_out, mode, Q, w, i_in, c_in, s_in, ids, scores, counts, unique, stats,
                                        None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(T=0), dict(T=17), dict(T=17, pool=1, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"fuse lists: needs 1 <= n_vecs <= 16", kw
    for kw in (dict(pool=0), dict(n_out=0), dict(n_out=17), dict(pool=86, n_out=86), dict(T=16, pool=17), dict(T=1, pool=257),
               dict(T=2, pool=0x80000000, n_out=1)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"fuse lists: needs 1 <= n_out <= pool and n_vecs * pool <= 256", kw
    for mode in (2, 7, 0xFFFFFFFF):
        assert call(mode=mode) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"fuse lists: the mode is HNSW_FUSE_SUM (0) or HNSW_FUSE_MIN (1)"
    assert call(T=16, pool=16, n_out=16, mode=1, Q=None) == _lib.ERR_ARG  # (within the limits: the pointer is refused)
    assert b"needs the vectors" in L.hnsw_last_error()
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse lists: at most 2^31 - 1 queries"
    for name in ("Q", "i_in", "ids", "scores"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == b"fuse lists: needs the vectors, the candidates' ids and the id and score outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse lists: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, T=0, pool=0, n_out=0, mode=9, Q=None, i_in=None, ids=None, scores=None, stats=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0


def test_search_argument_errors_need_no_device():
    index = small()
    T = 3
    Q = rand_vectors(6 * T, D, 12).reshape(6, T, D)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h=index, Q=Q, nq=6, T=T, w=None, mode=0, n=4, pool=20, ef=32, ids="own"):
        o_ids = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_s, o_c, o_u = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full(6, 9, dtype=np.uint32), np.full(6, 8, dtype=np.uint32)
        code = L.hnsw_search_batch_multi(None if h is None else h._h, ptr(Q, f32p), nq, T, ptr(w, f32p), mode, n, pool, ef,
                                         ptr(o_ids, u32p), ptr(o_s, f32p), ptr(o_c, u32p), ptr(o_u, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_s == 3.5).all() and (o_c == 9).all() and (o_u == 8).all()
            assert o_ids is None or (o_ids == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    for kw in (dict(T=0), dict(T=17, pool=4)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"multi search: needs 1 <= n_vecs <= 16", kw
    for kw in (dict(pool=0), dict(n=0), dict(n=21), dict(pool=86), dict(T=16, pool=17), dict(T=1, pool=257, n=257)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"multi search: needs 1 <= n <= pool and n_vecs * pool <= 256", kw
    assert rc(mode=2) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"multi search: the mode is HNSW_FUSE_SUM (0) or HNSW_FUSE_MIN (1)"
    assert rc(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"multi search: needs queries, an id buffer and at most 2^31 - 1 vectors in all"
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(nq=(1 << 31) // 3 + 1) == _lib.ERR_ARG
    assert b"2^31 - 1 vectors" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle)
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, pool=0, n=0, T=0, mode=5) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    after = {k: index.stat(k) for k in KEYS}
    assert after == before and index.stat("uploads") == 0
    # the candidate call's limit while ids are deleted
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65, n=4) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"multi search: needs pool <= 64 while ids are deleted"
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(12, D, 12).reshape(6, 2, D)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_multi(Q[:, :, :5], 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:
        index.search_batch_multi(Q[:, 0], 3, 10, 32)  # [nq, dim]: not a multi-vector call
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_multi(Q, 3, 10, 32, weights=np.ones((6, 3)))
    with pytest.raises(ValueError):
        index.search_batch_multi(Q, 3, 10, 32, mode="max")
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_multi(Q, 11, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_multi(Q, 3, 129, 32)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_multi(Q[:0], 3, 10, 32, mode="min")  # nq == 0
    assert got[0].shape == got[1].shape == (0, 3) and got[2].shape == got[3].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.fuse_lists_device(4, 2, 10, 11, "sum", 256, None, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.fuse_lists_device(0, 2, 10, 3, "min", None, None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("multi_calls", "multi_fuse_launches"):
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
            "float": C.c_float, "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 17 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 14
    for define, value in (("HNSW_MULTI_MAX_VECS", H.MULTI_MAX_VECS), ("HNSW_FUSE_MAX_CANDS", H.FUSE_MAX_CANDS),
                          ("HNSW_FUSE_SUM", H.FUSE_SUM), ("HNSW_FUSE_MIN", H.FUSE_MIN)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert (H.MULTI_MAX_VECS, H.FUSE_MAX_CANDS, H.FUSE_SUM, H.FUSE_MIN, H.DIVERSE_POOL_MAX) == (16, 256, 0, 1, 256)
    for method in ("search_batch_multi", "fuse_lists_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.fuse_lists)
