"""hnsw_search_batch_filtered_multi on the host: pack_allow_many's layout, and everything the entry point decides
before it touches the device (argument errors, n == 0, nq == 0, the ef' limit of the graph path).  None of these needs
a GPU -- which is the point: they pass on a machine without one."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import rand_vectors

N, D = 600, 12


# ---- pack_allow_many ------------------------------------------------------------------------------------------
def stacked(masks, n_points):
    rows = [H.pack_allow(m, n_points) for m in masks]
    assert len({b for _, b in rows}) == 1
    return np.stack([w for w, _ in rows]), rows[0][1]


@pytest.mark.parametrize("bits", [64, 128, 100, 1, 63, 65, 700, 500])  # multiples of 64 and not; above and below N
def test_pack_allow_many_bool_rows(bits):
    rng = np.random.default_rng(bits)
    m2d = rng.random((5, bits)) < 0.4
    m2d[3] = False  # an empty mask
    want_w, want_b = stacked(list(m2d), N)
    for given in (m2d, list(m2d), tuple(np.array(r) for r in m2d)):
        words, b = H.pack_allow_many(given, N)
        assert b == want_b == bits
        assert words.dtype == np.uint64 and words.shape == (5, max(1, (bits + 63) // 64)) and words.flags.c_contiguous
        assert np.array_equal(words, want_w)
    assert not words[3].any()
    # bit i & 63 of word i >> 6, stated once more without pack_allow
    for g in range(5):
        for i in range(bits):
            assert ((int(words[g, i >> 6]) >> (i & 63)) & 1) == int(m2d[g, i])


def test_pack_allow_many_id_lists():
    lists = [np.array([0, 63, 64, 599]), np.array([], dtype=np.int64), [5], np.array([7, 700, 3])]  # 700 >= n_points
    words, b = H.pack_allow_many(lists, N)
    want_w, want_b = stacked(lists, N)
    assert b == want_b == N and words.shape == (4, (N + 63) // 64) and np.array_equal(words, want_w)
    assert not words[1].any()
    assert [i for i in range(N) if (int(words[3, i >> 6]) >> (i & 63)) & 1] == [3, 7]


def test_pack_allow_many_single_mask_and_mixed_lengths():
    m = np.random.default_rng(3).random(130) < 0.5
    words, b = H.pack_allow_many([m], N)
    assert words.shape == (1, 3) and b == 130 and np.array_equal(words[0], H.pack_allow(m, N)[0])
    words, b = H.pack_allow_many(m.reshape(1, -1), N)
    assert words.shape == (1, 3) and b == 130
    with pytest.raises(ValueError):
        H.pack_allow_many([m, m[:100]], N)  # the masks of one call share allow_bits
    with pytest.raises(ValueError):
        H.pack_allow_many([], N)


def test_the_gpu_tests_masks_allow_what_their_plan_assumes():
    """tests/test_gpu_filtered_multi.py plans its mixed calls on these counts: three masks far above a
    filter_exact_max of 50, three far below"""
    from tests import filtered_restate as FR
    from tests.test_gpu_filtered import masks
    sizes = [int(FR.allowed_ids_of(*H.pack_allow(m, 1000), 1000).size) for _, m in masks(1000, 5)]
    assert sizes == [1000, 521, 107, 4, 1, 0]


def test_mask_none_is_exported():
    assert H.MASK_NONE == 0xFFFFFFFF == _lib.MASK_NONE
    assert "hnsw_search_batch_filtered_multi" in _lib.SYMBOLS


# ---- decided before the device is touched ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    vs = rand_vectors(N, D, 11)
    index = H.HNSW.new(8, 32, D, H.VEC_F32).insert_bulk(vs, 2, False, levels=O.draw_levels(N, 8, 11))
    return index, rand_vectors(6, D, 12)


def raw_call(index, Q, nq, n, ef, words, n_masks, bits, mask_of, ids="own", counts=None):
    """the C entry with every pointer under the test's control -> (status, ids, counts)"""
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    out_ids = np.full((max(nq, 1), max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
    rc = _lib.lib().hnsw_search_batch_filtered_multi(index._h, ptr(Q, f32p), nq, n, ef, ptr(words, u64p), n_masks, bits,
                                                     ptr(mask_of, u32p), ptr(out_ids, u32p), None, ptr(counts, u32p),
                                                     None, None)
    return rc, out_ids


def test_argument_errors_need_no_device(small):
    index, Q = small
    rng = np.random.default_rng(5)
    words, bits = H.pack_allow_many(rng.random((3, N)) < 0.5, N)
    mo = np.array([0, 1, 2, H.MASK_NONE, 0, 1], dtype=np.uint32)
    nq = 6
    up0 = index.stat("uploads")

    def rc(**kw):
        a = dict(Q=Q, nq=nq, n=5, ef=32, words=words, n_masks=3, bits=bits, mask_of=mo)
        a.update(kw)
        return raw_call(index, a["Q"], a["nq"], a["n"], a["ef"], a["words"], a["n_masks"], a["bits"], a["mask_of"],
                        ids=a.get("ids", "own"))[0]

    assert rc(Q=None) == _lib.ERR_ARG
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(mask_of=None) == _lib.ERR_ARG
    assert rc(words=None) == _lib.ERR_ARG                       # masks NULL, allow_bits > 0, a query names a mask
    assert rc(words=None, n_masks=0) == _lib.ERR_ARG            # ... and with n_masks 0 the names are out of range
    assert rc(mask_of=np.array([0, 1, 3, 0, 0, 0], dtype=np.uint32)) == _lib.ERR_ARG   # 3 is not < n_masks
    assert rc(mask_of=np.array([0, 1, 0xFFFFFFFE, 0, 0, 0], dtype=np.uint32)) == _lib.ERR_ARG
    assert rc(n_masks=2) == _lib.ERR_ARG                        # row 2 is named
    assert rc(n=65) == _lib.ERR_ARG
    assert rc(n=300, ef=10) == _lib.ERR_ARG
    # (refused before Q, mask_of or ids are touched, and before anything is sized by nq)
    assert rc(nq=1 << 31, ids=np.zeros((6, 5), dtype=np.uint32)) == _lib.ERR_ARG
    assert index.stat("uploads") == up0
    assert index.stat("filtered_multi_calls") == 0 and index.stat("filtered_multi_masks") == 0


def test_nq_zero_and_n_zero_return_ok(small):
    index, Q = small
    words, bits = H.pack_allow_many(np.ones((2, N), dtype=bool), N)
    mo = np.array([0, 1, H.MASK_NONE, 1, 0, 0], dtype=np.uint32)
    assert raw_call(index, Q, 0, 5, 32, words, 2, bits, mo)[0] == _lib.OK
    assert raw_call(index, None, 0, 5, 32, None, 0, 0, None, ids=None)[0] == _lib.OK
    counts = np.full(6, 9, dtype=np.uint32)
    rc, ids = raw_call(index, Q, 6, 0, 32, words, 2, bits, mo, counts=counts)
    assert rc == _lib.OK and (counts == 0).all() and (ids == 7).all()  # counts zeroed, ids untouched
    # every query without a mask: no masks at all is legal (n == 0, so still nothing is launched)
    none = np.full(6, H.MASK_NONE, dtype=np.uint32)
    counts[:] = 9
    assert raw_call(index, Q, 6, 0, 32, None, 0, 0, none, counts=counts)[0] == _lib.OK and (counts == 0).all()
    ids, dists, counts, stats, paths = index.search_batch_filtered_multi(Q, 0, 32, np.ones((2, N), dtype=bool), [0, 1, -1, 1, 0, 0])
    assert ids.shape == (6, 0) and (counts == 0).all()
    assert index.stat("uploads") == 0


def test_ef_above_the_graph_paths_limit(small):
    index, Q = small
    masks = np.ones((2, N), dtype=bool)
    index.set_option("filter_exact_max", -1)  # every mask is planned on the graph path
    try:
        for n, ef in ((10, 257), (1, 1000)):
            with pytest.raises(H.HnswError) as e:
                index.search_batch_filtered_multi(Q, n, ef, masks, [0, 1, -1, 1, 0, 0])
            assert e.value.code == _lib.ERR_ARG, (n, ef)
        with pytest.raises(H.HnswError) as e:  # ... also when no query has a mask
            index.search_batch_filtered_multi(Q, 10, 257, None, [-1] * 6)
        assert e.value.code == _lib.ERR_ARG
    finally:
        index.set_option("filter_exact_max", 65536)  # the default
    assert index.stat("uploads") == 0


def test_python_mirror_checks_mask_of(small):
    index, Q = small
    masks = np.ones((2, N), dtype=bool)
    with pytest.raises(ValueError):
        index.search_batch_filtered_multi(Q, 5, 32, masks, [0, 1])  # one entry per query
    with pytest.raises(ValueError):
        index.search_batch_filtered_multi(Q, 5, 32, masks, [0, 1, -2, 0, 0, 0])
    with pytest.raises(H.HnswError) as e:
        index.search_batch_filtered_multi(Q, 5, 32, masks, [0, 1, 2, 0, 0, 0])
    assert e.value.code == _lib.ERR_ARG
