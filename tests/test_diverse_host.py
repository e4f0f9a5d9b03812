"""Diversified search on the host (include/hnsw_mi355x.h, "diversified search"): the numpy restatement of the selection
(hnsw_rs_amd.diverse.mmr_select) against a second, deliberately plain one (tests/diverse_cases.py) bit for bit, the
pair distance's symmetry, and everything hnsw_diversify_device and hnsw_search_batch_diverse decide before they touch a
device -- every argument error with its message, nq == 0, the stat keys, the exported symbols and their prototypes.
None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import diverse_cases as DC
from tests.util import oracle_from_product, rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_diversify_device", "hnsw_search_batch_diverse")
KEYS = ("uploads", "diverse_calls", "diverse_launches", "filtered_range_calls", "filtered_set_calls",
        "filtered_set_range_calls", "filtered_queries_graph", "filtered_queries_exact")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("pool", DC.POOLS)
def test_mmr_select_is_the_plain_loop_bit_for_bit(pool):
    pd = DC.grid_pair_dist()
    seen_zero_gap = seen_short = False
    for with_counts in (True, False):
        ids, dists, counts, statuses = DC.synthetic_lists(pool, with_counts, seed=100 * pool + with_counts)
        for n_out in DC.n_outs(pool):
            k = DC.n_queries(pool, n_out)
            cut = lambda a: None if a is None else a[:k]  # noqa: E731
            for lam in DC.LAMBDAS:
                what = "pool=%d counts=%s n_out=%d lambda=%g" % (pool, with_counts, n_out, lam)
                got = H.mmr_select(cut(ids), cut(dists), cut(counts), cut(statuses), pd, lam, n_out)
                want = DC.naive(cut(ids), cut(dists), cut(counts), cut(statuses), pd, lam, n_out)
                DC.assert_diverse_equal(got, want, what)
                assert np.array_equal(got[4], want[4]) and np.array_equal(got[4], cut(statuses)), what
                assert got[0].shape == got[1].shape == got[2].shape == (k, n_out) and got[3].shape == (k,)
                # the planted queries did what they are there for
                assert got[3][0] == 0 and (got[0][0] == MAX).all() and np.isposinf(got[1][0]).all()
                assert got[3][4] == 0 and (got[0][4] == MAX).all() and got[4][4] == DC.ERR_NAN_INPUT
                assert np.isposinf(got[2][:, 0]).all()  # the first hit has no hit before it
                sel = got[0] != MAX
                assert not np.isnan(got[1][sel]).any()  # a NaN distance is never selected
                if pool >= 3 and 0 < lam < 1:
                    assert got[3][1] == n_out and got[3][3] == n_out
                    assert got[3][2] == min(n_out, pool - 1), what  # (the NaN entry alone is left over)
                if lam == 0:  # 0 * inf is NaN: neither the NaN nor the +inf distance can be selected
                    assert not np.isposinf(got[1][sel]).any()
                seen_zero_gap |= bool((got[2][sel] == 0).any())
                seen_short |= bool((got[3] < n_out).any())
    assert seen_short and (seen_zero_gap or pool < 32)


@pytest.mark.parametrize("pool", DC.POOLS)
def test_lambda_one_is_the_first_entries_by_distance_then_position(pool):
    pd = DC.grid_pair_dist()
    for with_counts in (True, False):
        ids, dists, counts, statuses = DC.synthetic_lists(pool, with_counts, seed=100 * pool + with_counts)
        for n_out in DC.n_outs(pool):
            got = H.mmr_select(ids, dists, counts, statuses, pd, 1.0, n_out)
            for q in range(DC.NQ):
                present = ids[q] != MAX if counts is None else np.arange(pool) < min(int(counts[q]), pool)
                if statuses[q] != 0:
                    present[:] = False
                j = np.flatnonzero(present & ~np.isnan(dists[q]))
                order = j[np.argsort(dists[q][j], kind="stable")][:n_out]  # (stable: ties by position; -0 == +0)
                assert got[3][q] == order.size, (pool, with_counts, n_out, q)
                assert np.array_equal(got[0][q, :order.size], ids[q][order])
                assert np.array_equal(got[1][q, :order.size].view(np.uint32), dists[q][order].view(np.uint32))
                assert (got[0][q, order.size:] == MAX).all() and np.isposinf(got[1][q, order.size:]).all()


def test_lambda_zero_walks_farthest_point_first():
    pd = DC.grid_pair_dist()
    ids, dists, counts, statuses = DC.synthetic_lists(64, True, seed=9)
    got = H.mmr_select(ids, dists, counts, statuses, pd, 0.0, 5)
    for q in (1, 3, 6):
        c = min(int(counts[q]), 64)
        if c < 2 or np.isinf(dists[q, :c]).any() or np.isnan(dists[q, :c]).any():
            continue
        assert got[0][q, 0] == ids[q, 0]  # every score is 0 at step 0: the first present position
        far = max(pd(int(ids[q, 0]), int(ids[q, j])) for j in range(1, c))
        assert got[2][q, 1] == far  # then the entry farthest from it


def test_mmr_select_refuses_shapes_beyond_the_limits_and_flags_ids_beyond_the_index():
    ids, dists = np.zeros((2, 300), dtype=np.uint32), np.zeros((2, 300), dtype=np.float32)
    pd = lambda a, b: np.float32(0)  # noqa: E731
    for a in ((ids, dists, None, None, pd, 0.5, 1), (ids[:, :10], dists[:, :10], None, None, pd, 0.5, 11),
              (ids[:, :10], dists[:, :10], None, None, pd, 0.5, 0), (ids[:, :10], dists[:, :9], None, None, pd, 0.5, 1),
              (ids[:, :10], dists[:, :10], None, None, pd, 1.5, 1), (ids[:, :10], dists[:, :10], None, None, pd, -0.1, 1),
              (ids[:, :10], dists[:, :10], None, None, pd, float("nan"), 1)):
        with pytest.raises(ValueError):
            H.mmr_select(*a)
    ids = np.arange(20, dtype=np.uint32).reshape(2, 10)
    for fn in (H.mmr_select, DC.naive):
        got = fn(ids, dists[:, :10], None, None, pd, 0.5, 3, n_points=15)
        assert got[4].tolist() == [0, DC.ERR_ARG] and got[3].tolist() == [3, 0] and (got[0][1] == MAX).all()
        got = fn(ids, dists[:, :10], np.array([10, 5], dtype=np.uint32), None, pd, 0.5, 3, n_points=15)
        assert got[4].tolist() == [0, 0] and got[3].tolist() == [3, 3]  # (the ids beyond the index are not present)


# ---- the pair distance: Point::dist2other is bit-symmetric for both kinds ---------------------------------------------
@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_pair_distance_is_bit_symmetric_and_the_oracles(kind):
    n = 400
    vs = rand_vectors(n, 23, 7)  # (23: a quantised row with a tail)
    vs[100:200] = vs[0:100]
    lv = O.draw_levels(n, 8, 7)
    index = H.HNSW.new(8, 32, 23, kind).insert_bulk(vs, 2, False, levels=lv)
    orc = oracle_from_product(index, vs, lv)
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    a[:100], b[:100] = np.arange(100), np.arange(100, 200)
    bits = lambda x: np.float32(x).view(np.uint32)  # noqa: E731
    for x, y in zip(a.tolist(), b.tolist()):
        d = bits(index.distance(x, y))
        assert d == bits(index.distance(y, x)) == bits(orc.distance(x, y)) == bits(orc.distance(y, x)), (x, y)
    assert all(index.distance(x, x + 100) == 0 for x in range(100))


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first

    def call(h=index._h, nq=6, pool=64, n_out=10, lam=0.5, i_in=fake, d_in=fake, c_in=fake, s_in=fake, ids=fake, dists=fake,
             gaps=fake, counts=fake, stats=fake):
        return L.hnsw_diversify_device(h, nq, pool, n_out, lam, i_in, d_in, c_in, s_in, ids, dists, gaps, counts, stats, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    for kw in (dict(pool=0), dict(pool=257), dict(n_out=0), dict(n_out=65), dict(pool=300, n_out=300)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"diversify: needs 1 <= n <= pool <= 256", kw
    for lam in (-0.001, 1.001, float("nan"), float("inf")):
        assert call(lam=lam) == _lib.ERR_ARG, lam
        assert L.hnsw_last_error() == b"diversify: lambda must lie in [0, 1]", lam
    assert call(pool=256, n_out=256, lam=1.0, i_in=None) == _lib.ERR_ARG  # (within the limits: the pointer is refused)
    assert b"needs the candidates" in L.hnsw_last_error()
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert b"2^31 - 1" in L.hnsw_last_error()
    for name in ("i_in", "d_in", "ids", "dists"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == b"diversify: needs the candidates' ids and distances and the id and distance outputs", name
    assert call(s_in=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"diversify: the stats output goes with the candidates' stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, pool=0, n_out=0, lam=7.0, i_in=None, d_in=None, ids=None, dists=None, gaps=None, stats=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0


def test_search_argument_errors_need_no_device():
    index, other = small(), small(seed=2)
    index.set_labels(np.arange(N, dtype=np.uint32) % 5)
    s, foreign = index.mask_set([np.ones(N, dtype=bool)]), other.mask_set([np.ones(N, dtype=bool)])
    Q = rand_vectors(6, D, 12)
    mo = np.zeros(6, dtype=np.uint32)
    lo, hi = np.zeros(6, dtype=np.uint32), np.full(6, 3, dtype=np.uint32)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()

    def rc(h=index, Q=Q, nq=6, n=4, pool=20, ef=32, lam=0.5, st=None, mo=None, lo=None, hi=None, ids="own"):
        o_ids = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_d, o_g, o_c = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full((6, max(n, 1)), 2.5, dtype=np.float32), \
            np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_diverse(None if h is None else h._h, ptr(Q, f32p), nq, n, pool, ef, lam,
                                           None if st is None else st._s, ptr(mo, u32p), ptr(lo, u32p), ptr(hi, u32p),
                                           ptr(o_ids, u32p), ptr(o_d, f32p), ptr(o_g, f32p), ptr(o_c, u32p), None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_d == 3.5).all() and (o_g == 2.5).all() and (o_c == 9).all()
            assert o_ids is None or (o_ids == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    for kw in (dict(pool=0), dict(pool=257), dict(n=0), dict(n=21), dict(n=300, pool=300)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"diverse search: needs 1 <= n <= pool <= 256", kw
    for lam in (-0.5, 1.5, float("nan")):
        assert rc(lam=lam) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"diverse search: lambda must lie in [0, 1]"
    assert rc(mo=mo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"diverse search: mask_of needs its mask set"
    assert rc(lo=lo) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"diverse search: a label range needs lo and hi, both or neither"
    assert rc(hi=hi) == _lib.ERR_ARG
    assert rc(st=foreign) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"diverse search: the mask set belongs to another handle"
    assert rc(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"diverse search: needs queries, an id buffer and at most 2^31 - 1 queries"
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(nq=1 << 31) == _lib.ERR_ARG
    # the candidate call's limits: pool <= 64 under a filter or while ids are deleted ...
    for kw in (dict(st=s), dict(lo=lo, hi=hi), dict(st=s, mo=mo, lo=lo, hi=hi)):
        assert rc(pool=65, **kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"diverse search: needs pool <= 64 under a filter or while ids are deleted"
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
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, pool=0, n=0, lam=9.0) == _lib.OK
    assert rc(nq=0, st=foreign) == _lib.ERR_ARG and rc(nq=0, mo=mo) == _lib.ERR_ARG
    after = {k: index.stat(k) for k in KEYS}
    assert after == before and index.stat("uploads") == 0
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65) == _lib.ERR_ARG
    assert b"pool <= 64" in L.hnsw_last_error()
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY
    for x in (s, foreign):
        x.close()


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(6, D, 12)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_diverse(Q[:, :5], 3, 10, 32)
    assert e.value.code == _lib.ERR_BAD_DIM
    with pytest.raises(ValueError):
        index.search_batch_diverse(Q, 3, 10, 32, lo=1)
    with pytest.raises(ValueError):
        index.search_batch_diverse(Q, 3, 10, 32, lo=[0, 1], hi=3)
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_diverse(Q, 11, 10, 32)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_diverse(Q, 3, 10, 32, lam=2.0)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_diverse(Q, 3, 10, 32, mask_of=[0] * 6)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_diverse(Q[:0], 3, 10, 32)  # nq == 0
    assert got[0].shape == got[1].shape == got[2].shape == (0, 3) and got[3].shape == (0,)
    with pytest.raises(H.HnswError) as e:
        index.diversify_device(4, 10, 11, 0.5, 256, 256, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.diversify_device(0, 10, 3, 0.5, None, None, None, None, None, None)  # nq == 0
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("diverse_calls", "diverse_launches"):
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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 15 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 16
    assert re.search(r"#define HNSW_DIVERSE_POOL_MAX 256\b", header) and H.DIVERSE_POOL_MAX == 256
    for method in ("search_batch_diverse", "diversify_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.mmr_select)
