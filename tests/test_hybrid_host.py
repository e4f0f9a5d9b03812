"""Hybrid search on the host (include/hnsw_mi355x.h, "hybrid search"): the numpy restatement of the rank fusion
(hnsw_rs_amd.hybrid.fuse_ranked) against a second, deliberately plain one (tests/hybrid_cases.py) bit for bit, and
everything hnsw_fuse_ranked_device and hnsw_search_batch_hybrid decide before they touch a device -- every argument error
with its message, nq == 0, the stat keys, the exported symbols and their prototypes.  None of this needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import hybrid_cases as HC
from tests.util import rand_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 12
MAX = 0xFFFFFFFF
f32p, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
NEW_SYMBOLS = ("hnsw_fuse_ranked_device", "hnsw_search_batch_hybrid")
KEYS = ("uploads", "hybrid_calls", "hybrid_fuse_launches")


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def small(n=N, kind=H.VEC_QUANT8, seed=1):
    vs = rand_vectors(n, D, seed)
    return H.HNSW.new(8, 32, D, kind).insert_bulk(vs, 2, False, levels=O.draw_levels(n, 8, seed))


def both(mode, rc, n_out, lists, w, ab, Q, dist, filt, k=HC.NQ):
    """fuse_ranked and the plain loop over the first k queries of a synthetic call"""
    cut = lambda a: None if a is None else a[:k]  # noqa: E731
    _, ids0, c0, st0, ext, sc, ce = lists
    f = None
    if filt is not None:
        f = {key: (cut(v) if key in ("mask_of", "lo", "hi") else v) for key, v in filt.items()}
    adm = None if f is None else H.filters_of(k, **HC.filters_args(f))
    args = (mode, rc, n_out, cut(ids0), cut(c0), cut(st0), cut(ext), cut(sc), cut(ce), cut(w), ab, cut(Q), dist)
    return H.fuse_ranked(*args, adm, HC.ID_SPAN), HC.naive(*args, f, HC.ID_SPAN)


# ---- the restatement against the plain one ----------------------------------------------------------------------------
@pytest.mark.parametrize("p0,E,W", HC.SHAPES)
def test_fuse_ranked_is_the_plain_loop_bit_for_bit(p0, E, W):
    dist = HC.table_dist()
    total = p0 + E * W
    dropped_somewhere = False
    for fk, with_counts in ((fk, wc) for fk in HC.FILTER_KINDS for wc in (True, False)):
        seed = 1000 * p0 + 100 * E + 10 * W + with_counts
        filt = HC.synthetic_filter(fk, seed)
        lists = HC.synthetic(p0, E, W, with_counts, seed, filt)
        Q = lists[0]
        for mode in (HC.RRF, HC.LINEAR):
            by_kind = {}
            for kind in HC.WEIGHT_KINDS:
                if fk not in ("none", "both") and kind == "ones":
                    continue
                w = HC.weights_of(kind, E, seed=p0 + E + W)
                for n_out in HC.n_outs(total) if fk in ("none", "both") else (min(10, total),):
                    # the planted queries alone where the plain loop is longest (the same properties, less Python time)
                    k = HC.N_PLANTED if total >= 150 and kind != "mixed" else HC.NQ
                    for use_q in ((True, False) if (mode == HC.RRF or E) and n_out == min(10, total) else (True,)):
                        what = "p0=%d E=%d W=%d filter=%s counts=%s mode=%d weights=%s n_out=%d Q=%s" % (
                            p0, E, W, fk, with_counts, mode, kind, n_out, use_q)
                        ab = HC.absent_of(E, seed + n_out)
                        got, want = both(mode, 60 if kind != "mixed" else 1, n_out, lists, w, ab, Q if use_q else None, dist,
                                         filt, k)
                        HC.assert_equal(got, want, what)
                        if not use_q:
                            assert got[2] is None
                            continue
                        by_kind[(kind, n_out)] = got
                        ids, scores, dists, counts, unique, dropped, st = got
                        assert ids.shape == scores.shape == dists.shape == (k, n_out), what
                        # the planted queries did what they are there for
                        assert st[0] == 0 and counts[0] == 0 and unique[0] == 0 and dropped[0] == 0 and (ids[0] == MAX).all()
                        if fk == "none":
                            assert unique[1] == max(p0, W if E else 0) and unique[2] == total, what
                            assert unique[3] <= total - (2 if (p0 or W) >= 3 else 0)
                            assert (dropped == 0).all()
                        if fk != "none" and HC.inadmissible_ids(filt, 5):
                            assert unique[5] == 0 and counts[5] == 0 and dropped[5] == total and st[5] == 0, what
                            assert dropped[4] >= (1 if p0 else 0) + E, what
                        assert st[6] == (HC.ERR_OVERFLOW if p0 else 0)
                        assert st[7] == HC.ERR_ARG and st[8] == HC.ERR_NAN_INPUT
                        if fk in ("set", "both"):
                            assert st[9] == HC.ERR_ARG
                        if fk in ("range", "both"):
                            assert st[10] == 0 and unique[10] == 0 and dropped[10] == total
                        for q in [6] * bool(p0) + [7, 8]:
                            assert counts[q] == 0 and unique[q] == 0 and dropped[q] == 0 and (ids[q] == MAX).all()
                            assert (scores[q] == (-np.inf if mode == HC.RRF else np.inf)).all() and np.isposinf(dists[q]).all()
                        sel = ids != MAX
                        assert not np.isnan(scores[sel]).any()  # a NaN score is never returned
                        assert (counts == sel.sum(axis=1)).all() and (counts <= unique).all()
                        dropped_somewhere |= bool(dropped.any())
                        for q in range(k):  # distinct ids, in the mode's (score, id) order
                            c = int(counts[q])
                            assert len(set(ids[q, :c].tolist())) == c
                            s, i = scores[q, :c] if mode == HC.LINEAR else -scores[q, :c], ids[q, :c].astype(np.int64)
                            assert all(s[a] < s[a + 1] or (s[a] == s[a + 1] and i[a] < i[a + 1]) for a in range(c - 1)), what
                        if kind == "mixed" and E == 0 and mode == HC.RRF and p0:  # a NaN weight is no error: every score is
                            assert st[13] == 0 and counts[13] == 0 and unique[13] == want[4][13]  # NaN, nothing is returned
            if fk in ("none", "both"):
                for n_out in HC.n_outs(total):  # no weights and weights of 1.0: the same bits, in BOTH modes
                    a, b = by_kind[("none", n_out)], by_kind[("ones", n_out)]
                    HC.assert_equal(a, tuple(x[:a[0].shape[0]] for x in b), "ones against none")
    assert dropped_somewhere


def explicit_dist(table):
    return lambda q_row, ids: np.array([table[int(i)] for i in ids], dtype=np.float32)


def test_rrf_by_hand():
    # dense [5, 9, 2], external [9, 7, 5, 9]: the second 9 is a repeat; k = 1
    ids0 = np.array([[5, 9, 2]], dtype=np.uint32)
    ext = np.array([[[9, 7, 5, 9]]], dtype=np.uint32)
    f = np.float32
    for fn in (H.fuse_ranked, HC.naive):
        ids, scores, dists, counts, unique, dropped, st = fn(HC.RRF, 1, 4, ids0, None, None, ext, None, None, None, None, None, None)
        # 5: 1/2 + 1/4, 9: 1/3 + 1/2, 2: 1/4, 7: 1/3
        assert ids[0].tolist() == [9, 5, 7, 2] and unique[0] == 4 and dropped[0] == 0 and counts[0] == 4 and dists is None
        assert scores[0].tolist() == [f(f(1) / f(3)) + f(0.5), f(0.75), f(f(1) / f(3)), f(0.25)]
        # 9 deleted: every later rank of both lists shifts, and the removal counts once per present entry
        adm = H.admissible_of(deleted=[9]) if fn is H.fuse_ranked else dict(deleted=[9])
        ids, scores, _, counts, unique, dropped, st = fn(HC.RRF, 1, 4, ids0, None, None, ext, None, None, None, None, None, None, adm)
        # 5: 1/2 + 1/3, 2: 1/3, 7: 1/2 -> 5, 7, 2
        assert ids[0].tolist() == [5, 7, 2, MAX] and unique[0] == 3 and dropped[0] == 3 and counts[0] == 3
        assert scores[0, :3].tolist() == [f(0.5) + f(f(1) / f(3)), f(0.5), f(f(1) / f(3))] and scores[0, 3] == -np.inf
        # equal scores go to the lower id: two disjoint lists
        ids, scores, *_ = fn(HC.RRF, 60, 4, np.array([[8, 3]], dtype=np.uint32), None, None,
                             np.array([[[4, 6]]], dtype=np.uint32), None, None, None, None, None, None)
        assert ids[0].tolist() == [4, 8, 3, 6]


def test_linear_by_hand_and_zero_signs():
    table = {5: 1.0, 9: 0.5, 2: 0.0, 7: 2.0}
    Q = np.zeros((1, 2), dtype=np.float32)
    ids0 = np.array([[5, 9]], dtype=np.uint32)
    ext = np.array([[[9, 7, 2]]], dtype=np.uint32)
    sc = np.array([[[4.0, 1.0, 0.0]]], dtype=np.float32)
    w = np.array([[1.0, -0.25]], dtype=np.float32)
    for fn in (H.fuse_ranked, HC.naive):
        got = fn(HC.LINEAR, 0, 4, ids0, None, None, ext, sc, None, w, np.array([2.0], dtype=np.float32), Q, explicit_dist(table))
        # 5: 1 - 0.5 (absent), 9: 0.5 - 1, 7: 2 - 0.25, 2: 0 + (-0.25 * 0 = -0) = 0
        assert got[0][0].tolist() == [9, 2, 5, 7] and got[1][0].tolist() == [-0.5, 0.0, 0.5, 1.75]
        assert got[2][0].tolist() == [0.5, 0.0, 1.0, 2.0]  # every hit's own distance
        # without Q the dense term is left out and the dense list only proposes: 5 -> -0.25 * 2, 9 -> -1, 7 -> -0.25, 2 -> -0
        got = fn(HC.LINEAR, 0, 4, ids0, None, None, ext, sc, None, w, np.array([2.0], dtype=np.float32), None, None)
        assert got[0][0].tolist() == [9, 5, 7, 2] and got[2] is None
        assert got[1][0].view(np.uint32).tolist()[3] == 0x80000000  # the fold's own bits: -0.0
        # -0 and +0 are one score: the id decides
        got = fn(HC.LINEAR, 0, 2, None, None, None, np.array([[[8, 3]]], dtype=np.uint32),
                 np.array([[[0.0, 0.0]]], dtype=np.float32), None, np.array([[1.0, -1.0]], dtype=np.float32), None, None, None)
        assert got[0][0].tolist() == [3, 8]


def test_fuse_ranked_refuses_shapes_beyond_the_limits():
    dist = HC.table_dist()
    ids0 = np.zeros((2, 8), dtype=np.uint32)
    ext = np.zeros((2, 2, 4), dtype=np.uint32)
    sc = np.zeros((2, 2, 4), dtype=np.float32)
    Q = np.zeros((2, 2), dtype=np.float32)
    base = dict(mode="rrf", rank_constant=60, n_out=4, ids0=ids0, counts0=None, statuses0=None, ext_ids=ext, ext_scores=sc,
                ext_counts=None, weights=None, absent=None, Q=Q, dist=dist)
    for kw in (dict(mode="sum"), dict(rank_constant=0), dict(rank_constant=(1 << 20) + 1), dict(n_out=0), dict(n_out=17),
               dict(ids0=None, ext_ids=None), dict(ext_ids=np.zeros((2, 8, 4), dtype=np.uint32)),
               dict(ids0=np.zeros((2, 250), dtype=np.uint32)), dict(mode="linear", ext_scores=None),
               dict(mode="linear", ext_ids=None, ext_scores=None, Q=None), dict(weights=np.ones((2, 2), dtype=np.float32))):
        with pytest.raises(ValueError):
            H.fuse_ranked(**dict(base, **kw))
    got = H.fuse_ranked(**dict(base, n_out=16))
    assert got[4].tolist() == [1, 1] and got[3].tolist() == [1, 1]
    with pytest.raises(ValueError):
        H.admissible_of(lo=1)
    with pytest.raises(ValueError):
        H.hybrid.mode_of("sum")


# ---- argument errors: decided before the device is touched -------------------------------------------------------------
def test_primitive_argument_errors_need_no_device():
    index = small()
    other = small(n=60)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    own_set, foreign = index.mask_set(np.ones((2, N), dtype=bool)), other.mask_set(np.ones((1, 60), dtype=bool))
    no_rows = index.mask_set(0, N)

    def call(h=index._h, nq=6, mode=0, rc=60, n_out=10, pool=16, i0=fake, c0=fake, s0=fake, E=2, W=8, e_ids=fake, e_sc=fake,
             e_cnt=fake, w=fake, ab=None, Q=fake, mset=None, mof=None, lo=None, hi=None, ids=fake, scores=fake, dists=fake,
             counts=fake, unique=fake, dropped=fake, stats=fake):
        return L.hnsw_fuse_ranked_device(h, nq, mode, rc, n_out, pool, i0, c0, s0, E, W, e_ids, e_sc, e_cnt, w, ab, Q, mset, mof,
                                         lo, hi, ids, scores, dists, counts, unique, dropped, stats, None)

    assert call(h=None) == _lib.ERR_ARG
    assert b"null handle" in L.hnsw_last_error()
    assert call(E=8, W=1) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: needs n_ext <= 7"
    for kw in (dict(i0=None, E=0), dict(i0=None, W=0), dict(pool=0, E=0), dict(pool=0, W=0)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"fuse ranked: needs at least one list: the dense one or an external one", kw
    for kw in (dict(n_out=0), dict(n_out=33), dict(pool=241), dict(E=7, W=37, i0=None), dict(i0=None, n_out=17),
               dict(pool=0x80000000), dict(W=0x80000000)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"fuse ranked: needs pool + n_ext * ext_width <= 256 and 1 <= n_out <= that total", kw
    for mode in (2, 7, 0xFFFFFFFF):
        assert call(mode=mode) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"fuse ranked: the mode is HNSW_HYBRID_RRF (0) or HNSW_HYBRID_LINEAR (1)"
    for rc in (0, (1 << 20) + 1):
        assert call(rc=rc) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"fuse ranked: reciprocal rank fusion needs 1 <= rank_constant <= 2^20"
    assert call(e_ids=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: needs the external lists' ids"
    assert call(mode=1, e_sc=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: the linear mode needs the external lists' scores"
    assert call(mode=1, E=0, Q=None, dists=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: the linear mode needs the queries or an external list"
    assert call(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: the distance output needs the queries"
    assert call(nq=1 << 31) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: at most 2^31 - 1 queries"
    for name in ("ids", "scores"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert L.hnsw_last_error() == b"fuse ranked: needs the id and score outputs", name
    assert call(s0=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: the stats output goes with the dense list's stats, both or neither"
    assert call(stats=None) == _lib.ERR_ARG
    assert b"both or neither" in L.hnsw_last_error()
    assert call(mset=foreign._s) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: the mask set belongs to another handle"
    assert call(mof=fake) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: mask_of needs its mask set"
    for kw in (dict(lo=fake), dict(hi=fake)):
        assert call(**kw) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"fuse ranked: a label range needs lo and hi, both or neither"
    assert call(mset=no_rows._s) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"fuse ranked: every query names row 0 of a set without rows"
    # nq == 0 is HNSW_OK whatever else is passed (but for the handle) and launches nothing
    assert call(nq=0) == _lib.OK
    assert call(nq=0, mode=9, rc=0, n_out=0, pool=0, i0=None, E=9, W=0, e_ids=None, ids=None, scores=None, stats=None) == _lib.OK
    assert call(nq=0, h=None) == _lib.ERR_ARG
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert call(h=empty._h) == _lib.ERR_EMPTY and call(h=empty._h, nq=0) == _lib.OK
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    del own_set


def test_search_argument_errors_need_no_device():
    index = small()
    other = small(n=60)
    Q = rand_vectors(6, D, 12)
    before = {k: index.stat(k) for k in KEYS}
    L = _lib.lib()
    foreign, no_rows = other.mask_set(np.ones((1, 60), dtype=bool)), index.mask_set(0, N)
    e_ids, e_sc = np.zeros((6, 2, 8), dtype=np.uint32), np.zeros((6, 2, 8), dtype=np.float32)
    some = np.zeros(6, dtype=np.uint32)

    def rc(h=index, Q=Q, nq=6, n=4, pool=20, ef=32, mode=0, k=60, E=2, W=8, e_ids=e_ids, e_sc=e_sc, w=None, mset=None, mof=None,
           lo=None, hi=None, ids="own"):
        o_ids = np.full((6, max(n, 1)), 7, dtype=np.uint32) if isinstance(ids, str) else ids
        o_s, o_c = np.full((6, max(n, 1)), 3.5, dtype=np.float32), np.full(6, 9, dtype=np.uint32)
        code = L.hnsw_search_batch_hybrid(None if h is None else h._h, ptr(Q, f32p), nq, n, pool, ef, mode, k, E, W,
                                          ptr(e_ids, u32p), ptr(e_sc, f32p), None, ptr(w, f32p), None, mset, ptr(mof, u32p),
                                          ptr(lo, u32p), ptr(hi, u32p), ptr(o_ids, u32p), ptr(o_s, f32p), None, ptr(o_c, u32p),
                                          None, None, None)
        if code != _lib.OK:  # an error leaves every output as it was
            assert (o_s == 3.5).all() and (o_c == 9).all()
            assert o_ids is None or (o_ids == 7).all()
        return code

    assert rc(h=None) == _lib.ERR_ARG
    assert rc(E=8, W=1) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs n_ext <= 7"
    assert rc(pool=0) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs pool >= 1"
    for kw in (dict(n=0), dict(n=37), dict(pool=241), dict(pool=32, E=7, W=33)):
        assert rc(**kw) == _lib.ERR_ARG, kw
        assert L.hnsw_last_error() == b"hybrid search: needs pool + n_ext * ext_width <= 256 and 1 <= n <= that total", kw
    assert rc(mode=2) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: the mode is HNSW_HYBRID_RRF (0) or HNSW_HYBRID_LINEAR (1)"
    for k in (0, (1 << 20) + 1):
        assert rc(k=k) == _lib.ERR_ARG
        assert L.hnsw_last_error() == b"hybrid search: reciprocal rank fusion needs 1 <= rank_constant <= 2^20"
    assert rc(e_ids=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs the external lists' ids"
    assert rc(mode=1, e_sc=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: the linear mode needs the external lists' scores"
    assert rc(Q=None) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs queries, an id buffer and at most 2^31 - 1 queries"
    assert rc(ids=None) == _lib.ERR_ARG
    assert rc(nq=1 << 31) == _lib.ERR_ARG
    assert b"2^31 - 1 queries" in L.hnsw_last_error()
    assert rc(mset=foreign._s) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: the mask set belongs to another handle"
    assert rc(mof=some) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: mask_of needs its mask set"
    assert rc(lo=some) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: a label range needs lo and hi, both or neither"
    assert rc(mset=no_rows._s) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: every query names row 0 of a set without rows"
    assert rc(pool=65, lo=some, hi=some) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs pool <= 64 under a filter or while ids are deleted"
    # nq == 0 is HNSW_OK whatever else is missing (but for the handle)
    assert rc(nq=0) == _lib.OK and rc(nq=0, Q=None, ids=None, pool=0, n=0, E=9, mode=5, k=0) == _lib.OK
    assert rc(nq=0, h=None) == _lib.ERR_ARG
    assert {k: index.stat(k) for k in KEYS} == before and index.stat("uploads") == 0
    index.mark_deleted(np.array([3, 5]))
    assert rc(pool=65) == _lib.ERR_ARG
    assert L.hnsw_last_error() == b"hybrid search: needs pool <= 64 under a filter or while ids are deleted"
    assert index.stat("uploads") == 0
    empty = H.HNSW.new(8, 32, D, H.VEC_F32)
    assert rc(h=empty) == _lib.ERR_EMPTY


def test_python_wrapper_argument_handling():
    index = small()
    Q = rand_vectors(6, D, 12)
    ext = np.zeros((6, 2, 8), dtype=np.uint32)
    with pytest.raises(H.HnswError) as e:
        index.search_batch_hybrid(Q[:, :5], 3, 10, 32, ext)
    assert e.value.code == _lib.ERR_BAD_DIM
    for kw in (dict(weights=np.ones(2)), dict(weights=np.ones((5, 3))), dict(mode="sum"), dict(ext_scores=np.zeros((6, 2, 7))),
               dict(lo=1)):
        with pytest.raises(ValueError):
            index.search_batch_hybrid(Q, 3, 10, 32, ext, **kw)
    with pytest.raises(ValueError):
        index.search_batch_hybrid(Q, 3, 10, 32, ext[:5])
    with pytest.raises(H.HnswError) as e:  # the library's own refusal, before any device
        index.search_batch_hybrid(Q, 27, 10, 32, ext)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(H.HnswError) as e:
        index.search_batch_hybrid(Q, 3, 10, 32, ext, mode="linear")  # (no scores)
    assert e.value.code == _lib.ERR_ARG
    got = index.search_batch_hybrid(Q[:0], 3, 10, 32, ext[:0], weights=[1.0, 0.5, 0.5])  # nq == 0; [1 + E] weights broadcast
    assert got[0].shape == got[1].shape == got[2].shape == (0, 3) and all(g.shape == (0,) for g in got[3:6])
    with pytest.raises(H.HnswError) as e:
        index.fuse_ranked_device(4, "rrf", 60, 27, 10, 256, None, None, 2, 8, 256, None, None, None, None, None, 256, 256)
    assert e.value.code == _lib.ERR_ARG
    index.fuse_ranked_device(0, "linear", 0, 3, 10, None, None, None, 0, 0, None, None, None, None, None, None, None, None)
    assert index.stat("uploads") == 0


# ---- the stat keys and the ABI ----------------------------------------------------------------------------------------
def test_stat_keys_exist_and_read_zero():
    index = small(n=50)
    for key in ("hybrid_calls", "hybrid_fuse_launches"):
        assert index.stat(key) == 0


def c_type_of(decl):
    """a parameter of a prototype -> the ctypes type the binding must use (device pointers d_*, the stream, the handle and
    the mask set are bound as void pointers)"""
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
    assert len(_lib.SYMBOLS[NEW_SYMBOLS[0]][1]) == 29 and len(_lib.SYMBOLS[NEW_SYMBOLS[1]][1]) == 26
    for define, value in (("HNSW_HYBRID_MAX_EXT", H.HYBRID_MAX_EXT), ("HNSW_HYBRID_RRF", H.HYBRID_RRF),
                          ("HNSW_HYBRID_LINEAR", H.HYBRID_LINEAR), ("HNSW_FUSE_MAX_CANDS", H.FUSE_MAX_CANDS)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert (H.HYBRID_MAX_EXT, H.HYBRID_RRF, H.HYBRID_LINEAR, H.FUSE_MAX_CANDS) == (7, 0, 1, 256)
    for method in ("search_batch_hybrid", "fuse_ranked_device"):
        assert hasattr(H.HNSW, method), method
    assert callable(H.fuse_ranked) and callable(H.admissible_of) and callable(H.filters_of)
    # the multi-vector block's "Not provided" points here, and this block has its own
    assert 'rank fusion (see "hybrid search" below' in header
    assert "min-max / z-score normalisation of scores" in header
