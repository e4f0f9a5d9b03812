"""Radius search on the host (include/hnsw_mi355x.h, "radius search"): the numpy restatement of the cut
(hnsw_rs_amd.radius.radius_cut) against a deliberately naive loop (tests/radius_cases.py) bit for bit, the ladder
(radius_ladder) over the CPU oracle's search with the coverage condition of the GPU test's worlds, and everything
hnsw_radius_cut_device and hnsw_search_batch_radius decide before they touch a device -- every argument error with its
message, nq == 0, the stat keys, the exported symbols and their prototypes.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import radius_cases as RC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_radius_cut_device", "hnsw_search_batch_radius")
KEYS = ("uploads", "radius_calls", "radius_rungs", "radius_launches", "deleted_queries_graph", "deleted_queries_exact")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the naive loop ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", RC.N_INS)
def test_radius_cut_is_the_naive_cut_bit_for_bit(n_in):
    for with_counts in (True, False):
        ids, dists, counts, stats, radius = RC.adversarial_lists(n_in, with_counts, seed=7 * n_in + with_counts)
        for n_out in sorted({n_in, 1024}):
            what = "n_in=%d counts=%s n_out=%d" % (n_in, with_counts, n_out)
            got = H.radius_cut(ids, dists, counts, stats, radius, n_out)
            RC.assert_cut_equal(got, RC.naive_cut(ids, dists, counts, stats, radius, n_out), what)
            assert got[0].shape == (RC.NQ, n_out) and got[2].shape == (RC.NQ,) and np.array_equal(got[4], stats)
            # the planted queries did what they are there for
            assert got[2][0] == n_in and got[3][0] == RC.MORE
            assert np.array_equal(got[0][0, :n_in], ids[0]) and np.array_equal(got[1][0, :n_in].view(np.uint32), dists[0].view(np.uint32))
            assert got[2][1] == (dists[1] == 0).sum() and (got[1][1, :got[2][1]] == 0).all()
            assert got[2][2] >= min(2, n_in) and (got[1][2, :got[2][2]] == radius[2]).sum() >= min(2, n_in)
            assert got[2][3] == 0 and got[3][3] == 0 and (got[0][3] == MAX).all() and np.isposinf(got[1][3]).all()
            assert got[2][4] == n_in - len(range(0, n_in, 3)) and got[3][4] == 0 and not np.isnan(got[1][4]).any()
            assert got[2][5] == 0 and got[3][5] == 0
            assert got[2][6] == 0 and got[2][7] == 0 and got[3][7] == 0
            for q in range(RC.NQ):  # padded behind the count, in input order before it
                assert (got[0][q, got[2][q]:] == MAX).all() and np.isposinf(got[1][q, got[2][q]:]).all()
        # without stats every query is an ordinary one
        got = H.radius_cut(ids, dists, counts, None, radius, n_in)
        RC.assert_cut_equal(got, RC.naive_cut(ids, dists, counts, None, radius, n_in), "no stats, n_in=%d" % n_in)
        assert got[4] is None


def test_radius_cut_refuses_shapes_beyond_the_limits():
    ids, dists = np.zeros((2, 1025), dtype=np.uint32), np.zeros((2, 1025), dtype=np.float32)
    for a in ((ids, dists, None, None, 1.0, 1025), (ids[:, :10], dists[:, :10], None, None, 1.0, 9),
              (ids[:, :10], dists[:, :10], None, None, 1.0, 1025), (ids[:, :10], dists[:, :9], None, None, 1.0, 10),
              (ids[:, :0], dists[:, :0], None, None, 1.0, 10)):
        with pytest.raises(ValueError):
            H.radius_cut(*a)


def test_to_csr_is_the_rows_behind_one_another():
    ids = np.array([[5, 6, MAX], [MAX, MAX, MAX], [1, 2, 3]], dtype=np.uint32)
    dists = np.array([[.5, .75, np.inf], [np.inf] * 3, [1, 2, 3]], dtype=np.float32)
    lims, f_ids, f_d = H.to_csr(ids, dists, np.array([2, 0, 3], dtype=np.uint32))
    assert lims.tolist() == [0, 2, 2, 5] and f_ids.tolist() == [5, 6, 1, 2, 3] and f_d.tolist() == [.5, .75, 1, 2, 3]
    with pytest.raises(ValueError):
        H.to_csr(ids, dists, np.array([2, 0, 4]))


# ---- the ladder over the oracle: what the GPU test expects, and that it covers every outcome ---------------------------
def naive_ladder(orc, Q, radius, n_first, max_n, ef):
    """THE LADDER one query at a time, through the naive cut"""
    rows = []
    for q in range(Q.shape[0]):
        k = 0
        while True:
            n_k = min(n_first << k, max_n)
            ids, dists, counts, stats = orc.search_batch(Q[q:q + 1], n_k, max(ef, n_k))
            c = RC.naive_cut(ids, dists, counts, None, radius[q:q + 1], max_n)
            if n_k == max_n or not c[3][0]:
                rows.append((c[0][0], c[1][0], c[2][0], c[3][0], k + 1, list(stats[0].astype(np.int64)) + [0]))
                break
            k += 1
    return tuple(np.array([r[i] for r in rows]) for i in range(6))


@pytest.mark.parametrize("name,kind", [("small", H.VEC_F32), ("small", H.VEC_QUANT8), ("lean", H.VEC_F32), ("ties", H.VEC_F32)])
def test_radius_ladder_over_the_oracle_covers_every_outcome(name, kind):
    _, _, orc, Q, radius = RC.world(name, kind)
    want = H.radius_ladder(lambda q, n, ef: orc.search_batch(q, n, ef, nthreads=8), Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_covered(want, "%s kind %d" % (name, kind))
    RC.assert_ladder_equal(want, naive_ladder(orc, Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF), name)
    ids, dists, counts, flags, rungs, stats = want
    assert rungs.min() == 1 and rungs.max() == 5 and set(rungs.tolist()) == {1, 2, 3, 4, 5}  # n = 8, 16, 32, 64, 128
    for q in range(64):
        w = counts[q]
        assert (dists[q, :w] <= radius[q]).all() and (ids[q, w:] == MAX).all()
        if flags[q]:
            assert w == RC.MAX_N and rungs[q] == 5
    if name == "ties":  # a stored row and its duplicate, both at distance 0 = the radius of query 0
        assert radius[0] == 0 and counts[0] == 2 and set(ids[0, :2].tolist()) == {0, 2800}


def test_radius_ladder_refuses_bad_arguments():
    search = lambda q, n, ef: (_ for _ in ()).throw(AssertionError("not reached"))
    Q = np.zeros((3, 4), dtype=np.float32)
    for kw in (dict(n_first=0), dict(n_first=9, max_n=8), dict(max_n=1025), dict(radius=-1.0), dict(radius=np.nan)):
        a = dict(radius=1.0, n_first=8, max_n=64, ef=0)
        a.update(kw)
        with pytest.raises(ValueError):
            H.radius_ladder(search, Q, a["radius"], a["n_first"], a["max_n"], a["ef"])


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_cut_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(nq=6, n_in=64, n_out=128, rad=fake, sel=None, n_sel=0, i_in=fake, d_in=fake, c_in=fake, s_in=fake, ids=fake,
             dists=fake, counts=fake, flags=fake, stats=fake):
        return L.hnsw_radius_cut_device(nq, n_in, n_out, rad, sel, n_sel, i_in, d_in, c_in, s_in, ids, dists, counts, flags,
                                        stats, None)

    for kw in (dict(n_in=0), dict(n_in=129), dict(n_out=1025), dict(n_in=1025, n_out=1025), dict(n_in=0, n_out=0)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert b"1 <= n_in <= n_out <= 1024" in L.hnsw_last_error(), kw
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert b"2^31 - 1" in L.hnsw_last_error()
    for name in ("rad", "i_in", "d_in", "ids", "dists"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert b"needs the radii" in L.hnsw_last_error(), name
    assert call(sel=fake, n_sel=7) == _lib.ERR_ARG
    assert b"selection names more queries" in L.hnsw_last_error()
    assert call(s_in=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed and launches nothing; so is an empty selection
    assert call(nq=0) == _lib.OK
    assert call(nq=0, n_in=0, n_out=0, rad=None, i_in=None, d_in=None, ids=None, dists=None, stats=None) == _lib.OK
    assert call(sel=fake, n_sel=0) == _lib.OK
    assert call(sel=fake, n_sel=0, n_in=0) == _lib.ERR_ARG  # (an empty selection does not excuse the limits)
    assert {k: index.stat(k) for k in KEYS} == before


def test_search_argument_errors_need_no_device():
    index = small()
    Q = rand_vectors(6, D, 12)
    rad = np.full(6, 0.5, dtype=np.float32)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h=index, Q=Q, nq=6, rad=rad, n_first=8, max_n=64, ef=16, ids="own"):
        o_ids = np.full((6, max(max_n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_d, o_c = np.full((6, max(max_n, 1)), 3.5, dtype=np.float32), np.full(6, 9, dtype=np.uint32)
        o_f, o_r = np.full(6, 9, dtype=np.uint32), np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_radius(None if h is None else h._h, ptr(Q, f32p), nq, ptr(rad, f32p), n_first, max_n, ef,
                                          ptr(o_ids, u32p), ptr(o_d, f32p), ptr(o_c, u32p), ptr(o_f, u32p), ptr(o_r, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_d == 3.5).all() and (o_c == 9).all() and (o_f == 9).all() and (o_r == 9).all()
            assert o_ids is None or (o_ids == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(n_first=0), dict(n_first=65), dict(max_n=1025, n_first=8), dict(max_n=0, n_first=0)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert b"1 <= n_first <= max_n <= 1024" in L.hnsw_last_error(), kw
    for kw in (dict(Q=None), dict(rad=None), dict(ids=None), dict(nq=1 << 31)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert b"needs queries, the radius of every query" in L.hnsw_last_error(), kw
    for bad, where in ((-0.5, 3), (np.nan, 5), (-np.inf, 0)):
        r = rad.copy()
        r[where] = bad
        assert rc(rad=r) == _lib.ERR_ARG, bad
        assert b"radius of query %d is negative or NaN" % where in L.hnsw_last_error(), bad
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, rad=None, ids=None, n_first=0, max_n=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before
    # the candidate call's limits while ids are deleted: max_n <= 64, and ef' <= 256 on the graph path
    index.mark_deleted(np.array([3, 5]))
    assert rc(max_n=65) == _lib.ERR_ARG
    assert b"max_n <= 64 while ids are deleted" in L.hnsw_last_error()
    after = {k: index.stat(k) for k in KEYS}
    assert after == before
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(6, D, 12)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_radius(Q[:, :5], 0.5)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_radius(Q, [0.5, 0.25])
    with pytest.raises(H.HnswError) as e:  # the library's own refusals, before any device
        index.search_batch_radius(Q, -1.0)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_radius(Q, 0.5, n_first=32, max_n=16)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_radius(Q[:0], 0.5, 8, 32)  # nq == 0
    assert got[0].shape == (0, 32) and got[2].shape == (0,) and got[5].shape == (0, 4)
    with pytest.raises(H.HnswError) as e:
        H.HNSW.radius_cut_device(4, 10, 9, 256, 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    H.HNSW.radius_cut_device(0, 10, 10, None, None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("radius_calls", "radius_rungs", "radius_launches"):
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
    return {"float*": f32p, "uint32_t*": u32p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 16 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 13
    assert re.search(r"#define HNSW_RADIUS_MAX_N 1024\b", header) and H.RADIUS_MAX_N == 1024
    assert re.search(r"#define HNSW_RADIUS_MORE\s+1u\b", header) and H.RADIUS_MORE == 1
    for method in ("search_batch_radius", "radius_cut_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.radius_cut) and callable(H.radius_ladder) and callable(H.to_csr)
