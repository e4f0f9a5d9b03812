"""hnsw_search_batch_filtered_ranges, _device, _device_finish and hnsw_count_labels_in_ranges on the host
(include/hnsw_mi355x.h, "label-SET filtered search"): the C prototypes against the ctypes binding, every argument error
the entry points decide before they touch a device, the planner's own count against numpy -- overlapping, adjacent,
duplicate, unsorted and empty members, the edges of the label space, label changes, deletions, inserts -- and the Python
wrapper's packing of ragged lists.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 3001, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_search_batch_filtered_ranges", "hnsw_search_batch_filtered_ranges_device",
               "hnsw_search_batch_filtered_ranges_device_finish", "hnsw_count_labels_in_ranges")
KEYS = ("uploads", "label_words_uploaded", "mask_set_words_uploaded", "filtered_ranges_calls", "filtered_ranges_groups",
        "filtered_range_calls", "filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- ABI ----------------------------------------------------------------------------------------------------------
def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use.  Device pointers (d_*), the stream and the
    handle are bound as void pointers: they are passed as integers or opaque handles, never as host arrays."""
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if name.startswith("d_") or kind in ("void*", "hnsw_index*"):
        assert kind.endswith("*"), decl
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "uint64_t*": C.POINTER(C.c_uint64), "hnsw_query_stats*": C.POINTER(_lib.QueryStats)}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    assert re.search(r"^#define HNSW_RANGES_MAX 16$", header, re.M) and _lib.RANGES_MAX == 16
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int
        assert [c_type_of(p) for p in params] == argtypes, name
    assert [len(_lib.SYMBOLS[s][1]) for s in NEW_SYMBOLS] == [13, 13, 14, 5]
    for method in ("search_batch_filtered_ranges", "search_batch_filtered_ranges_device",
                   "search_batch_filtered_ranges_device_finish", "count_labels_in_ranges"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.pack_ranges)
    index = small(n=50)
    for key in ("filtered_ranges_calls", "filtered_ranges_groups"):
        assert index.stat(key) == 0


# ---- argument errors: decided before the device is touched, the outputs left as they were -----------------------------
def raw(index, Q, nq, n, ef, K, lo, hi, ids="own", counts=None, dists=None):
    out_ids = np.full((max(nq, 1), max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
    rc = _lib.lib().hnsw_search_batch_filtered_ranges(index._h, ptr(Q, f32p), nq, n, ef, K, ptr(lo, u32p), ptr(hi, u32p),
                                                      ptr(out_ids, u32p), ptr(dists, f32p), ptr(counts, u32p), None, None)
    return rc, out_ids


def test_host_form_argument_errors_need_no_device():
    index = small(n=700)
    index.set_labels(np.arange(700, dtype=np.uint32) % 5)
    Q = rand_vectors(6, D, 12)
    lo, hi = H.pack_ranges([[1], [2, (3, 4)], [], [(0, MAX)], [0, 1, 2], [(4, 1), 3]])
    assert lo.shape == (6, 3)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(**kw):
        a = dict(Q=Q, nq=6, n=5, ef=32, K=3, lo=lo, hi=hi)
        a.update(kw)
        counts, dists = np.full(6, 9, dtype=np.uint32), np.full((6, max(a["n"], 1)), 3.5, dtype=np.float32)
        code, ids = raw(index, a["Q"], a["nq"], a["n"], a["ef"], a["K"], a["lo"], a["hi"], ids=a.get("ids", "own"),
                        counts=counts, dists=dists)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (counts == 9).all() and (dists == 3.5).all() and (ids is None or (ids == 7).all()), kw
        return code

    assert rc(Q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(lo=None) == _lib.ERR_ARG
    assert b"label ranges" in L.hnsw_last_error()
    assert rc(hi=None) == _lib.ERR_ARG
    assert rc(K=0) == _lib.ERR_ARG
    assert b"label ranges per query" in L.hnsw_last_error()
    assert rc(K=17) == _lib.ERR_ARG and rc(K=MAX) == _lib.ERR_ARG
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    assert rc(nq=1 << 31, K=1, ids=np.full((6, 5), 7, dtype=np.uint32)) == _lib.ERR_ARG
    # nq == 0 is HNSW_OK whatever else is missing; n == 0 zeroes the counts and launches nothing
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, lo=None, hi=None, K=0) == _lib.OK
    counts = np.full(6, 9, dtype=np.uint32)
    code, ids = raw(index, Q, 6, 0, 32, 3, lo, hi, counts=counts)
    assert code == _lib.OK and (counts == 0).all() and (ids == 7).all()
    assert raw(index, Q, 6, 0, 32, 3, lo, hi, counts=None)[0] == _lib.OK  # counts are optional
    # ef' = 257 with a list planned on the graph path (every one is, under -1): refused by the planner, on the host
    index.set_option("filter_exact_max", -1)
    assert rc(ef=257) == _lib.ERR_ARG and rc(n=1, ef=1000) == _lib.ERR_ARG
    assert b"graph path" in L.hnsw_last_error()
    index.set_option("filter_exact_max", 65536)
    assert {k: index.stat(k) for k in KEYS} == before  # no device, no upload, no call completed
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert raw(empty, Q, 6, 5, 32, 3, lo, hi)[0] == _lib.ERR_EMPTY


def test_device_forms_argument_errors_need_no_device():
    index = small(n=700)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    for fn, tail in ((L.hnsw_search_batch_filtered_ranges_device, ()),
                     (L.hnsw_search_batch_filtered_ranges_device_finish, (None,))):
        def call(h=index._h, dq=fake, nq=6, n=5, ef=32, K=3, lo=fake, hi=fake, ids=fake, stats=fake):
            return fn(h, dq, nq, n, ef, K, lo, hi, ids, None, None, stats, None, *tail)
        assert call(dq=None) == _lib.ERR_ARG
        assert call(lo=None) == _lib.ERR_ARG
        assert b"label ranges" in L.hnsw_last_error()
        assert call(hi=None) == _lib.ERR_ARG
        assert call(ids=None) == _lib.ERR_ARG
        assert call(stats=None) == _lib.ERR_ARG
        assert call(K=0) == _lib.ERR_ARG and call(K=17) == _lib.ERR_ARG
        assert call(nq=1 << 31) == _lib.ERR_ARG
        assert call(n=65, ef=65) == _lib.ERR_ARG
        assert call(ef=257) == _lib.ERR_ARG  # every query takes the graph path
        assert call(dq=None, nq=0, lo=None, hi=None, ids=None, stats=None) == _lib.OK  # nq == 0
        assert call(n=0, dq=None, lo=None, hi=None, ids=None, stats=None) == _lib.OK  # n == 0: nothing launched
        assert call(h=None) != _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before


def test_count_argument_errors():
    index = small(n=50)
    L = _lib.lib()
    one, out = np.array([1], dtype=np.uint32), C.c_uint64(99)
    assert L.hnsw_count_labels_in_ranges(None, ptr(one, u32p), ptr(one, u32p), 1, C.byref(out)) == _lib.ERR_ARG
    assert L.hnsw_count_labels_in_ranges(index._h, ptr(one, u32p), ptr(one, u32p), 1, None) == _lib.ERR_ARG
    assert L.hnsw_count_labels_in_ranges(index._h, None, ptr(one, u32p), 1, C.byref(out)) == _lib.ERR_ARG
    assert L.hnsw_count_labels_in_ranges(index._h, ptr(one, u32p), None, 1, C.byref(out)) == _lib.ERR_ARG
    big = np.zeros(17, dtype=np.uint32)
    assert L.hnsw_count_labels_in_ranges(index._h, ptr(big, u32p), ptr(big, u32p), 17, C.byref(out)) == _lib.ERR_ARG
    assert out.value == 99
    assert L.hnsw_count_labels_in_ranges(index._h, None, None, 0, C.byref(out)) == _lib.OK and out.value == 0


# ---- the planner's count ---------------------------------------------------------------------------------------------
LISTS = (
    [3], [(3, 3)], [(0, 0)], [(2, 17)],                      # single
    [(1, 5), (4, 9)], [(0, 40), (10, 20)],                   # overlapping
    [(1, 2), (3, 4)], [(3, 4), (1, 2), 5],                   # adjacent: [1, 4], [1, 5]
    [7, 7, 7], [(2, 6), (2, 6)],                             # duplicates
    [(30, 40), (0, 2), 11, (9, 10)],                         # unsorted
    [(5, 2)], [(5, 2), (1, 0)], [(9, 3), 4, (1, 0)], [],     # empty members, all empty, none
    list(range(16)), [2 * j for j in range(16)],             # k = 16
    [(0, MAX)], [(0, 5), (6, MAX)], [(1, MAX), 0],           # everything, in one member or two that touch
    [MAX, MAX - 1], [(MAX - 1, MAX - 1), (MAX, MAX)], [(MAX, MAX), (0, 0)], [(MAX - 1, MAX), (0, 1)],
)


def numpy_count(lab, alive, ranges):
    m = np.zeros(lab.shape[0], dtype=bool)
    for x in ranges:
        l, h = (x, x) if isinstance(x, int) else x
        m |= (lab >= l) & (lab <= h)  # (nothing when l > h)
    return int((m & alive).sum())


def test_count_labels_in_ranges_equals_numpy():
    index = small()
    rng = np.random.default_rng(11)
    lab = rng.integers(0, 41, size=N).astype(np.uint32)
    lab[[0, 1, 2, 1500, 3000]] = 0
    lab[[9, 10, 2999]] = MAX
    lab[[11, 12]] = MAX - 1
    alive = np.ones(N, dtype=bool)

    def check(what):
        for r in LISTS:
            assert index.count_labels_in_ranges(r) == numpy_count(lab, alive, r), (what, r)

    assert index.count_labels_in_ranges([(0, MAX)]) == N and index.count_labels_in_ranges([0]) == N  # no label set yet
    index.set_labels(lab)
    check("labels")
    deleted = rng.choice(N, 200, replace=False)
    deleted[:3] = [9, 0, 11]  # some at the edges of the label space
    deleted = np.unique(deleted)
    index.mark_deleted(deleted)
    alive[deleted] = False
    check("deleted")
    assert index.count_labels_in_ranges([(0, MAX)]) == N - deleted.size
    ids = rng.choice(N, 300, replace=False)
    lab[ids] = rng.integers(0, 41, size=300).astype(np.uint32)
    index.set_labels(lab[ids], ids)
    check("set_labels")
    back = deleted[::2]
    index.unmark_deleted(back)
    alive[back] = True
    check("unmark_deleted")
    # an insert: the new id has label 0
    assert index.insert_vec(rand_vectors(1, D, 77)[0], level=0) == N
    lab, alive = np.concatenate([lab, [0]]).astype(np.uint32), np.concatenate([alive, [True]])
    check("insert")
    assert index.count_labels_in_ranges([0]) == numpy_count(lab, alive, [0]) > 0
    for key in ("uploads", "label_words_uploaded", "filtered_ranges_calls"):  # no GPU, and no search
        assert index.stat(key) == 0, key


def test_the_planner_counts_a_list_exactly():
    """ef' = 257 is refused (HNSW_ERR_ARG, "graph path") iff the call's one list is planned on the graph path, and that is
    decided before the device is touched: the refusal flips exactly between filter_exact_max = A - 1 and A, A the size of
    the union -- members that overlap, repeat or touch counted once -- under deletions.  (At A the planner passes the call
    on: HNSW_OK with a GPU, a device error without one -- anything but HNSW_ERR_ARG.)"""
    index = small(n=700)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 12, size=700).astype(np.uint32)
    lab[[5, 6]] = MAX
    index.set_labels(lab)
    deleted = np.array([5, 17, 300, 599, 650])
    index.mark_deleted(deleted)
    alive = np.ones(700, dtype=bool)
    alive[deleted] = False
    Q = rand_vectors(1, D, 3)
    for r in ([3], [(1, 5), (4, 9)], [(1, 2), (3, 4)], [7, 7, (9, 3)], [11, (0, 1), 5], [(MAX, MAX), (MAX - 1, MAX - 1), 0],
              list(range(0, 12, 3)) + [(1, 0)] * 12):
        A = numpy_count(lab, alive, r)
        assert A > 0 and index.count_labels_in_ranges(r) == A
        lo, hi = H.pack_ranges([r])
        for exact_max, refused in ((A - 1, True), (A, False)):
            index.set_option("filter_exact_max", exact_max)
            rc, _ = raw(index, Q, 1, 1, 257, lo.shape[1], lo, hi)
            assert (rc == _lib.ERR_ARG) == refused, (r, A, exact_max, rc)
            if refused:
                assert b"graph path" in _lib.lib().hnsw_last_error()


# ---- the Python wrapper --------------------------------------------------------------------------------------------
def test_pack_ranges_pads_ragged_lists():
    lo, hi = H.pack_ranges([[1, (2, 3)], [], [5], [(7, 4), 0, MAX]])
    assert lo.dtype == hi.dtype == np.uint32 and lo.flags["C_CONTIGUOUS"] and hi.flags["C_CONTIGUOUS"]
    assert lo.tolist() == [[1, 2, 1], [1, 1, 1], [5, 1, 1], [7, 0, MAX]]
    assert hi.tolist() == [[1, 3, 0], [0, 0, 0], [5, 0, 0], [4, 0, MAX]]
    lo, hi = H.pack_ranges([[], []])  # K is at least 1
    assert lo.tolist() == [[1], [1]] and hi.tolist() == [[0], [0]]
    lo, hi = H.pack_ranges([[np.uint32(4), np.array([1, 2])]], 1)
    assert lo.tolist() == [[4, 1]] and hi.tolist() == [[4, 2]]
    with pytest.raises(ValueError):
        H.pack_ranges([[1], [2]], 3)  # one list per query
    with pytest.raises(ValueError):
        H.pack_ranges([[-1]])
    with pytest.raises(ValueError):
        H.pack_ranges([[(0, 2 ** 32)]])


def test_python_wrapper_argument_handling():
    index = small(n=700)
    Q = rand_vectors(6, D, 12)
    lists = [[1], [2, (3, 4)], [], [(0, MAX)], [0, 1, 2], [(4, 1), 3]]
    got = index.search_batch_filtered_ranges(Q, 0, 32, lists)  # n == 0 launches nothing: the wrapper alone runs
    assert got[0].shape == (6, 0) and got[1].shape == (6, 0) and (got[2] == 0).all() and got[4].shape == (6,)
    with pytest.raises(ValueError):
        index.search_batch_filtered_ranges(Q, 5, 32, lists[:2])
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_ranges(Q[:, :5], 5, 32, lists)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:  # 17 members: the library's error, before any device
        index.search_batch_filtered_ranges(Q, 5, 32, [list(range(17))] * 6)
    assert e.value.code == _lib.ERR_ARG
    assert index.count_labels_in_ranges([]) == 0 and index.count_labels_in_ranges([(3, 1)]) == 0
    with pytest.raises(H.HnswError):
        index.count_labels_in_ranges(list(range(17)))
    for key in ("uploads", "filtered_ranges_calls", "label_words_uploaded"):
        assert index.stat(key) == 0, key
