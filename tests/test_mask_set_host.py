"""hnsw_mask_set on the host: create / write / update / read / count against numpy bitsets, the masked tail word, the
errors that leave a set unchanged, and everything hnsw_search_batch_filtered_set (and the device form) decides before
it touches the device.  None of this needs a GPU -- managing a set never does."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import rand_vectors

N, D = 600, 12
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def small():
    vs = rand_vectors(N, D, 11)
    index = H.HNSW.new(8, 32, D, H.VEC_F32).insert_bulk(vs, 2, False, levels=O.draw_levels(N, 8, 11))
    return index, rand_vectors(6, D, 12)


def packed(bits_row):
    """a bool row -> its words, stated without pack_allow: id i at bit i & 63 of word i >> 6"""
    w = np.zeros((len(bits_row) + 63) // 64, dtype=np.uint64)
    for i in np.flatnonzero(bits_row):
        w[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return w


def rows_of(s):
    return [s.read(g).copy() for g in range(s.n_masks)]


# ---- round trips ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [640, 576, 100, 601, 1, 63, 65, 1000, 4096])  # multiples of 64 and not; beyond len
def test_create_write_update_read_count_round_trip(small, bits):
    index, _ = small
    rng = np.random.default_rng(bits)
    m = rng.random((4, bits)) < 0.3
    m[2] = False
    s = index.mask_set(m)
    assert (s.n_masks, s.allow_bits) == (4, bits)
    for g in range(4):
        assert np.array_equal(s.read(g), packed(m[g])) and s.count(g) == int(m[g].sum())
    # a set of empty rows, filled by write and update
    e = index.mask_set(3, n_points=bits)
    assert (e.n_masks, e.allow_bits) == (3, bits)
    assert all(not e.read(g).any() and e.count(g) == 0 for g in range(3))
    e.write(0, m[0])                       # a bool row
    e.write(1, np.flatnonzero(m[1]))       # an id list
    e.write(2, packed(m[3]))               # packed words
    for g, src in ((0, 0), (1, 1), (2, 3)):
        assert np.array_equal(e.read(g), packed(m[src])) and e.count(g) == int(m[src].sum())
    # update: set some, clear some, against the numpy bitset
    ref = m[0].copy()
    on = rng.choice(bits, min(bits, 40), replace=False)
    e.update(0, on)
    ref[on] = True
    assert np.array_equal(e.read(0), packed(ref)) and e.count(0) == int(ref.sum())
    off = rng.choice(bits, min(bits, 25), replace=False)
    e.update(0, off, allow=False)
    ref[off] = False
    assert np.array_equal(e.read(0), packed(ref)) and e.count(0) == int(ref.sum())
    assert np.array_equal(e.read(1), packed(m[1]))  # the other rows are untouched
    e.write(0, np.zeros(bits, dtype=bool))
    assert e.count(0) == 0
    s.close()
    e.close()
    e.close()  # (idempotent)


def test_create_from_id_lists_takes_the_index_length(small):
    index, _ = small
    s = index.mask_set([np.array([0, 63, 64, 599]), np.array([], dtype=np.int64), [5]])
    assert (s.n_masks, s.allow_bits) == (3, N)
    assert [s.count(g) for g in range(3)] == [4, 0, 1]
    big = index.mask_set([[1, 2, 700]], n_points=1024)  # room for later inserts
    assert big.allow_bits == 1024 and big.count(0) == 3


@pytest.mark.parametrize("bits", [100, 601, 65])
def test_bits_of_the_tail_word_are_masked(small, bits):
    index, _ = small
    W = (bits + 63) // 64
    ones = np.full(W, np.uint64(0xFFFFFFFFFFFFFFFF))
    L = _lib.lib()
    h = C.c_void_p()
    both = np.concatenate([ones, ones])
    assert L.hnsw_mask_set_create(index._h, 2, bits, ptr(both, u64p), C.byref(h)) == _lib.OK
    want = packed(np.ones(bits, dtype=bool))
    assert want[-1] != ones[-1]
    out = np.zeros(W, dtype=np.uint64)
    cnt = C.c_uint64()
    for g in (0, 1):
        assert L.hnsw_mask_set_read(h, g, ptr(out, u64p)) == _lib.OK and np.array_equal(out, want)
        assert L.hnsw_mask_set_count(h, g, C.byref(cnt)) == _lib.OK and cnt.value == bits
    zeros = np.zeros(W, dtype=np.uint64)
    assert L.hnsw_mask_set_write(h, 1, ptr(zeros, u64p)) == _lib.OK
    assert L.hnsw_mask_set_write(h, 1, ptr(ones, u64p)) == _lib.OK
    assert L.hnsw_mask_set_read(h, 1, ptr(out, u64p)) == _lib.OK and np.array_equal(out, want)
    L.hnsw_mask_set_free(h)


def test_update_is_idempotent(small):
    index, _ = small
    s = index.mask_set(2, n_points=300)
    ids = np.array([0, 5, 5, 64, 299, 128, 5])
    s.update(1, ids)
    once = rows_of(s)
    s.update(1, ids)
    assert all(np.array_equal(a, b) for a, b in zip(once, rows_of(s))) and s.count(1) == 5
    s.update(1, [5, 5], allow=False)
    s.update(1, [5], allow=False)
    assert s.count(1) == 4 and not s.read(0).any()
    s.update(1, [])  # nothing to do
    assert s.count(1) == 4


def test_update_errors_leave_the_set_unchanged(small):
    index, _ = small
    rng = np.random.default_rng(9)
    s = index.mask_set(rng.random((3, 200)) < 0.5)
    before = rows_of(s)
    for row, ids in ((1, [3, 7, 200]), (1, [200]), (1, [3, 0xFFFFFFFF]), (3, [3]), (0xFFFFFFFF, [3])):
        for allow in (True, False):
            with pytest.raises(H.HnswError) as e:
                s.update(row, ids, allow=allow)
            assert e.value.code == _lib.ERR_ARG
            assert all(np.array_equal(a, b) for a, b in zip(before, rows_of(s)))
    for call in (lambda: s.read(3), lambda: s.count(3), lambda: s.write(3, np.zeros(200, dtype=bool))):
        with pytest.raises(H.HnswError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG
    assert all(np.array_equal(a, b) for a, b in zip(before, rows_of(s)))
    L = _lib.lib()
    assert L.hnsw_mask_set_update(None, 0, None, 0, 1) == _lib.ERR_ARG
    assert L.hnsw_mask_set_info(None, None, None) == _lib.ERR_ARG
    assert L.hnsw_mask_set_create(None, 1, 64, None, C.byref(C.c_void_p())) == _lib.ERR_ARG
    L.hnsw_mask_set_free(None)  # (like free)


def test_sets_need_no_device_and_no_points(small):
    """a set is made on an empty handle too (allow_bits is the caller's), and nothing here uploads anything"""
    index = H.HNSW.new(8, 32, D, H.VEC_F32).insert_bulk(rand_vectors(80, D, 3), 1, False)
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    s = empty.mask_set(2, n_points=128)
    s.update(0, [1, 127])
    assert s.count(0) == 2
    zero = index.mask_set(0)  # no rows: legal, HNSW_MASK_NONE queries can still name it
    assert (zero.n_masks, zero.allow_bits) == (0, 80)
    nobits = index.mask_set(2, n_points=0)  # rows without words: nothing is allowed
    assert nobits.read(1).shape == (0,) and nobits.count(1) == 0
    for key in ("uploads", "mask_set_words_uploaded", "mask_set_recounts", "mask_set_compactions", "filtered_set_calls"):
        assert index.stat(key) == 0, key
    index.set_option("mask_set_cache_mb", 0)
    index.set_option("mask_set_cache_mb", 64)
    with pytest.raises(H.HnswError):
        index.set_option("mask_set_cache_mb", -1)


# ---- hnsw_search_batch_filtered_set: decided before the device is touched ----------------------------------------
def raw_set(index, Q, nq, n, ef, s, mask_of, ids="own", counts=None):
    out_ids = np.full((max(nq, 1), max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
    rc = _lib.lib().hnsw_search_batch_filtered_set(index._h, ptr(Q, f32p), nq, n, ef, s, ptr(mask_of, u32p),
                                                   ptr(out_ids, u32p), None, ptr(counts, u32p), None, None)
    return rc, out_ids


def test_set_search_argument_errors_need_no_device(small):
    index, Q = small
    rng = np.random.default_rng(5)
    s = index.mask_set(rng.random((3, N)) < 0.5)
    other = H.HNSW.new(8, 32, D, H.VEC_F32).insert_bulk(rand_vectors(50, D, 2), 1, False)
    foreign = other.mask_set(rng.random((3, N)) < 0.5)
    mo = np.array([0, 1, 2, H.MASK_NONE, 0, 1], dtype=np.uint32)
    keys = ("uploads", "mask_set_words_uploaded", "mask_set_recounts", "filtered_set_calls", "filtered_multi_calls")
    before = {k: index.stat(k) for k in keys}

    def rc(**kw):
        a = dict(Q=Q, nq=6, n=5, ef=32, s=s._s, mask_of=mo)
        a.update(kw)
        return raw_set(index, a["Q"], a["nq"], a["n"], a["ef"], a["s"], a["mask_of"], ids=a.get("ids", "own"))[0]

    assert rc(s=None) == _lib.ERR_ARG
    assert b"needs a mask set" in _lib.lib().hnsw_last_error()
    assert rc(s=foreign._s) == _lib.ERR_ARG                     # a set of another handle
    assert b"another handle" in _lib.lib().hnsw_last_error()
    assert raw_set(other, Q, 6, 5, 32, s._s, mo)[0] == _lib.ERR_ARG
    assert rc(Q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(mask_of=np.array([0, 1, 3, 0, 0, 0], dtype=np.uint32)) == _lib.ERR_ARG   # 3 is not < n_masks
    assert rc(mask_of=np.array([0, 1, 0xFFFFFFFE, 0, 0, 0], dtype=np.uint32)) == _lib.ERR_ARG
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    assert rc(nq=1 << 31, ids=np.zeros((6, 5), dtype=np.uint32)) == _lib.ERR_ARG
    assert rc(nq=1 << 31, mask_of=None, ids=np.zeros((6, 5), dtype=np.uint32)) == _lib.ERR_ARG
    norows = index.mask_set(0)
    assert rc(s=norows._s, mask_of=None) == _lib.ERR_ARG        # NULL mask_of names row 0, which it does not have
    assert rc(s=norows._s) == _lib.ERR_ARG
    # the device form: the same set checks, and its own limits, before any device pointer is looked at
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    for fn, tail in ((L.hnsw_search_batch_filtered_device, ()), (L.hnsw_search_batch_filtered_device_finish, (None,))):
        assert fn(index._h, fake, 6, 5, 32, None, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 32, foreign._s, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, None, 6, 5, 32, s._s, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 32, s._s, None, None, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 32, s._s, None, fake, None, None, None, None, *tail) == _lib.ERR_ARG  # d_stats
        assert fn(index._h, fake, 6, 65, 65, s._s, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 257, s._s, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, fake, 6, 5, 32, norows._s, None, fake, None, None, fake, None, *tail) == _lib.ERR_ARG
        assert fn(index._h, None, 0, 5, 32, s._s, None, None, None, None, None, None, *tail) == _lib.OK  # nq == 0
    assert {k: index.stat(k) for k in keys} == before


def test_set_search_nq_zero_and_n_zero_return_ok(small):
    index, Q = small
    s = index.mask_set(np.ones((2, N), dtype=bool))
    mo = np.array([0, 1, H.MASK_NONE, 1, 0, 0], dtype=np.uint32)
    before = index.stat("uploads"), index.stat("mask_set_words_uploaded")
    assert raw_set(index, Q, 0, 5, 32, s._s, mo)[0] == _lib.OK
    assert raw_set(index, None, 0, 5, 32, s._s, None, ids=None)[0] == _lib.OK
    counts = np.full(6, 9, dtype=np.uint32)
    rc, ids = raw_set(index, Q, 6, 0, 32, s._s, mo, counts=counts)
    assert rc == _lib.OK and (counts == 0).all() and (ids == 7).all()  # counts zeroed, ids untouched
    ids, dists, counts, stats, paths = index.search_batch_filtered_set(Q, 0, 32, s, [0, 1, -1, 1, 0, 0])
    assert ids.shape == (6, 0) and (counts == 0).all()
    ids, dists, counts, stats, paths = index.search_batch_filtered_set(Q, 0, 32, s)  # mask_of None: row 0
    assert ids.shape == (6, 0) and (counts == 0).all()
    assert (index.stat("uploads"), index.stat("mask_set_words_uploaded")) == before


def test_set_search_ef_above_the_graph_paths_limit(small):
    index, Q = small
    s = index.mask_set(np.ones((2, N), dtype=bool))
    uploads = index.stat("uploads")
    index.set_option("filter_exact_max", -1)  # every row is planned on the graph path
    try:
        for n, ef in ((10, 257), (1, 1000)):
            with pytest.raises(H.HnswError) as e:
                index.search_batch_filtered_set(Q, n, ef, s, [0, 1, -1, 1, 0, 0])
            assert e.value.code == _lib.ERR_ARG, (n, ef)
    finally:
        index.set_option("filter_exact_max", 65536)  # the default
    assert index.stat("uploads") == uploads


def test_python_mirror_checks_mask_of(small):
    index, Q = small
    s = index.mask_set(np.ones((2, N), dtype=bool))
    with pytest.raises(ValueError):
        index.search_batch_filtered_set(Q, 5, 32, s, [0, 1])  # one entry per query
    with pytest.raises(ValueError):
        index.search_batch_filtered_set(Q, 5, 32, s, [0, 1, -2, 0, 0, 0])
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_set(Q, 5, 32, s, [0, 1, 2, 0, 0, 0])
    assert e.value.code == _lib.ERR_ARG


def test_symbols_are_declared_and_exported():
    names = ["hnsw_mask_set_create", "hnsw_mask_set_free", "hnsw_mask_set_info", "hnsw_mask_set_write",
             "hnsw_mask_set_update", "hnsw_mask_set_read", "hnsw_mask_set_count", "hnsw_search_batch_filtered_set",
             "hnsw_search_batch_filtered_device", "hnsw_search_batch_filtered_device_finish"]
    L = C.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert H.MaskSet is not None and hasattr(H.HNSW, "mask_set")
