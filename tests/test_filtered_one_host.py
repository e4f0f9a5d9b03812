"""hnsw_search_filtered, the one-query filtered search whose concurrent callers are gathered, without a GPU: the symbols
and their prototypes, every argument error (decided before the device is touched, on a handle that never uploaded), n == 0,
the option "filter_exact_grouped" and the new counters.  (The kernels' resources are held by
tests/test_filtered_set_range_host.py and tests/test_filtered_kernel_resources.py, the kernels' homes by
tests/test_kernel_matrix_complete.py: the grouped form adds arguments to three kernels and no kernel.)"""
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
N, D = 700, 12
MAX = 0xFFFFFFFF
NONE = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
KEYS = ("uploads", "label_words_uploaded", "mask_set_words_uploaded", "filtered_one_calls", "filtered_one_batches",
        "filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact", "filtered_range_calls",
        "filtered_set_range_calls", "coalesced_queries", "coalesced_batches")


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def test_argument_errors_need_no_device():
    index, other = small(), small(seed=2)
    index.set_labels(np.arange(N, dtype=np.uint32) % 3)
    rng = np.random.default_rng(5)
    s = index.mask_set([rng.random(N) < 0.5, rng.random(N) < 0.2])
    foreign = other.mask_set([np.ones(N, dtype=bool)])
    q = rand_vectors(1, D, 12)[0]
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h="own", q=q, n=5, ef=32, st=None, row=NONE, lo=0, hi=MAX, ids="own", count="own", want_count=9):
        out_ids = np.full(max(n, 1), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        dists = np.full(max(n, 1), 3.5, dtype=np.float32)
        cnt, path = C.c_uint32(9), C.c_uint8(9)
        code = L.hnsw_search_filtered(index._h if h == "own" else h, ptr(q, f32p), n, ef, None if st is None else st._s, row, lo,
                                      hi, ptr(out_ids, u32p), ptr(dists, f32p), C.byref(cnt) if count == "own" else None,
                                      C.byref(path))
        # an argument error leaves every output as it was
        assert (dists == 3.5).all() and path.value == 9 and (out_ids is None or (out_ids == 7).all())
        assert cnt.value == want_count
        return code

    assert rc(h=None) == _lib.ERR_ARG
    assert rc(q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(count=None) == _lib.ERR_ARG
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    for row in (0, 1, 5, MAX - 1):  # a row without a set
        assert rc(row=row) == _lib.ERR_ARG, row
        assert b"mask set" in L.hnsw_last_error()
    assert rc(st=foreign, row=0) == _lib.ERR_ARG
    assert b"another handle" in L.hnsw_last_error()
    assert rc(st=foreign, row=NONE) == _lib.ERR_ARG
    for row in (2, 3, MAX - 1):  # neither < n_masks nor HNSW_MASK_NONE
        assert rc(st=s, row=row) == _lib.ERR_ARG, row
        assert b"names mask" in L.hnsw_last_error()
    # n == 0: *count = 0, nothing launched, with and without a set
    assert rc(n=0, want_count=0) == _lib.OK
    assert rc(n=0, st=s, row=1, lo=1, hi=2, want_count=0) == _lib.OK
    assert rc(n=0, st=s, row=NONE, want_count=0) == _lib.OK
    after = {k: index.stat(k) for k in KEYS}
    assert after == before and after["uploads"] == 0  # the handle has never uploaded
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    cnt = C.c_uint32(9)
    ids = np.full(5, 7, dtype=np.uint32)
    assert L.hnsw_search_filtered(empty._h, ptr(q, f32p), 5, 32, None, NONE, 0, MAX, ptr(ids, u32p), None, C.byref(cnt),
                                  None) == _lib.ERR_EMPTY
    for x in (s, foreign):
        x.close()


def test_the_bench_entry_refuses_what_it_cannot_run():
    index = small()
    L = _lib.lib()
    Q = rand_vectors(4, D, 3)
    lo, hi = np.zeros(4, dtype=np.uint32), np.full(4, MAX, dtype=np.uint32)
    ids = np.zeros((4, 5), dtype=np.uint32)
    rows = np.zeros(4, dtype=np.uint32)

    def call(Q=Q, nq=4, n=5, threads=2, lo=lo, hi=hi, ids=ids, st=None, row=None):
        return L.hnsw_bench_search_filtered_threads(index._h, ptr(Q, f32p), nq, n, 32, st, ptr(row, u32p), ptr(lo, u32p),
                                                    ptr(hi, u32p), threads, 0.0, ptr(ids, u32p), None, None, None, None, None,
                                                    None, None)

    for kw in (dict(Q=None), dict(nq=0), dict(n=0), dict(threads=0), dict(threads=4097), dict(lo=None), dict(hi=None),
               dict(ids=None), dict(row=rows)):  # (rows without a set)
        assert call(**kw) == _lib.ERR_ARG, kw
    s = index.mask_set([np.ones(N, dtype=bool)])
    assert call(st=s._s) == _lib.ERR_ARG  # a set without rows
    s.close()
    assert index.stat("uploads") == 0


def test_filter_exact_grouped_is_0_or_1():
    index = small(n=50)
    index.set_option("filter_exact_grouped", 1)
    index.set_option("filter_exact_grouped", 0)
    for bad in (2, -1, 100):
        with pytest.raises(H.HnswError) as e:
            index.set_option("filter_exact_grouped", bad)
        assert e.value.code == _lib.ERR_ARG


def c_type_of(decl):
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    name = re.search(r"(\w+)$", decl).group(1)
    kind = decl[: -len(name)].replace("const", "").replace(" ", "")
    if kind in ("void*", "hnsw_index*", "hnsw_mask_set*"):
        return C.c_void_p
    return {"float*": f32p, "uint32_t*": u32p, "uint8_t*": u8p, "uint64_t*": C.POINTER(C.c_uint64), "int32_t*": C.POINTER(C.c_int32),
            "double*": C.POINTER(C.c_double), "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}[kind]


def test_symbols_are_exported_and_prototypes_match_the_binding():
    header = open(os.path.join(ROOT, "include", "hnsw_mi355x.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for name, n_args in (("hnsw_search_filtered", 12), ("hnsw_bench_search_filtered_threads", 19)):
        assert hasattr(L, name), name
        m = re.search(r"^int %s\((.*?)\);" % name, header, re.S | re.M)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == n_args
        assert [c_type_of(p) for p in params] == argtypes, name
    for method in ("search_filtered", "search_filtered_threads"):
        assert hasattr(H.HNSW, method), method
    index = small(n=50)
    for key in ("filtered_one_calls", "filtered_one_batches"):
        assert index.stat(key) == 0


def test_python_wrapper_argument_handling():
    index = small(n=50)
    with pytest.raises(H.HnswError) as e:
        index.search_filtered(np.zeros(D + 1, dtype=np.float32), 5, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(H.HnswError) as e:
        index.search_filtered(np.zeros(D, dtype=np.float32), 5, 32, row=0)  # a row without a set
    assert e.value.code == _lib.ERR_ARG
    ids, dists, count, path = index.search_filtered(np.zeros(D, dtype=np.float32), 0, 32)
    assert ids.shape == (0,) and dists.shape == (0,) and count == 0
    assert index.stat("uploads") == 0
