"""Grouped search on the GPU (include/hnsw_mi355x.h, "grouped search"), held to the numpy restatement of the collapse
(hnsw_rs_amd.grouped.group_by_label; tests/test_grouped_host.py holds that to a naive one).  All comparisons are on ids,
distance BITS, group labels, sizes and counts:
  1. hnsw_group_by_label_device alone over synthetic device lists (no search), the host test's sweep and more;
  2. the unfiltered search: search_batch_grouped is group_by_label of search_batch(Q, pool, ef) of the same handle, and,
     once, of the CPU oracle's search;
  3. the filtered searches (a range, a set row, both, HNSW_MASK_NONE), with the exact path forced for some groups, under
     deletions, and with a NaN query;
  4. label changes between two calls are seen;
  5. launch accounting with the kernel log."""
import ctypes as C
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import grouped_cases as GC
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
N, D, M, NQ = 3000, 16, 8, 128
KINDS = [H.VEC_F32, H.VEC_QUANT8]
f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def world_labels():
    lab = (np.arange(N) % 37).astype(np.uint32)
    lab[100:500] = 5  # a hot label: its group overflows per_group
    return lab


@functools.lru_cache(maxsize=None)
def world(kind):
    """the index of a kind with its labels, rows, queries and two rows of a mask set's bits (built once, shared; a test
    that changes labels or deletes ids puts them back)"""
    vs, lv, Q = rand_vectors(N, D, 31), O.draw_levels(N, M, 31), rand_vectors(NQ, D, 32)
    index = H.HNSW.new(M, 32, D, kind).insert_bulk(vs, 4, False, levels=lv)
    index.set_labels(world_labels())
    rng = np.random.default_rng(33)
    rows_b = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.2])
    for a in (vs, lv, Q, rows_b):
        a.setflags(write=False)
    return index, vs, lv, Q, rows_b


def up(a):  # (uint32 travels as int32: the bits are what the kernel reads)
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.float32 else a.view(np.int32)).to(torch.device("cuda:0"))


def collapse_on_device(index, ids, dists, counts, stats, G, P, want_counts=True):
    """hnsw_group_by_label_device over uploaded lists -> (ids, dists, labels, sizes, counts or None, stats or None), log"""
    import torch
    dev = torch.device("cuda:0")
    nq, pool = ids.shape
    d_in = up(ids), up(dists), None if counts is None else up(counts), None if stats is None else up(stats.astype(np.uint32))
    o_ids = torch.full((nq, G, P), 7, dtype=torch.int32, device=dev)
    o_dists = torch.full((nq, G, P), 3.5, dtype=torch.float32, device=dev)
    o_lab = torch.full((nq, G), 7, dtype=torch.int32, device=dev)
    o_sz = torch.full((nq, G), 7, dtype=torch.int32, device=dev)
    o_counts = torch.full((nq,), 9, dtype=torch.int32, device=dev) if want_counts else None
    o_stats = None if stats is None else torch.full((nq, 4), 5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.group_by_label_device(nq, pool, G, P, d_in[0], d_in[1], d_in[2], d_in[3], o_ids, o_dists, o_lab, o_sz, o_counts,
                                    o_stats, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    u = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
    return (u(o_ids), o_dists.cpu().numpy(), u(o_lab), u(o_sz), u(o_counts),
            None if o_stats is None else o_stats.cpu().numpy().astype(np.int64)), log


# ---- 1. the primitive alone --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def column_index():
    """a small index whose label column is the synthetic lists' (tests/grouped_cases.py), and one without labels"""
    vs, lv = rand_vectors(GC.N_LABELS, D, 41), O.draw_levels(GC.N_LABELS, M, 41)
    index = H.HNSW.new(M, 32, D, H.VEC_F32).insert_bulk(vs, 2, False, levels=lv)
    index.set_labels(GC.column())
    return index, H.HNSW.new(M, 32, D, H.VEC_F32).insert_bulk(vs, 2, False, levels=lv)


@pytest.mark.parametrize("pool", GC.POOLS)
def test_primitive_alone_is_the_restatement_bit_for_bit(pool):
    index, unlabelled = column_index()
    labels = GC.column()
    launches = index.stat("grouped_launches")
    n_calls = 0
    shapes = GC.shapes(pool) + ([(32, 32), (256, 4), (4, 256)] if pool == 256 else [])  # n_groups * per_group = 1024
    for with_counts in (True, False):  # (False: d_counts_in is NULL, presence by the pad id, pads in the middle)
        ids, dists, counts = GC.synthetic_lists(pool, with_counts, seed=100 * pool + with_counts)
        stats = np.random.default_rng(pool).integers(2 ** 31, 2 ** 32, (GC.NQ, 4)).astype(np.int64)
        stats[:, 3] = 0
        stats[8, 3] = _lib.ERR_NAN_INPUT  # a failed query: count 0, padded rows, its record kept
        blank_ids, blank_counts = ids.copy(), None if counts is None else counts.copy()
        if with_counts:
            blank_counts[8] = 0
        else:
            blank_ids[8] = MAX
        for G, P in shapes:
            what = "pool=%d counts=%s G=%d P=%d" % (pool, with_counts, G, P)
            got, log = collapse_on_device(index, ids, dists, counts, stats, G, P)
            n_calls += 1
            assert log.get("hx_filt_merge_kernel") == 1, (what, dict(log))
            if n_calls > 1:  # (the first call may have brought the label column to HBM)
                assert dict(log) == {"hx_filt_merge_kernel": 1}, (what, dict(log))
            want = H.group_by_label(blank_ids, dists, blank_counts, labels, G, P)
            GC.assert_grouped_equal(got, want, what)
            want_stats = stats.copy()
            want_stats[:, :3] &= 0xFFFFFFFF
            got[5][:, :3] &= 0xFFFFFFFF
            assert np.array_equal(got[5], want_stats), what
            assert got[4][8] == 0 and (got[0][8] == MAX).all() and np.isposinf(got[1][8]).all()
            assert (got[2][8] == 0).all() and (got[3][8] == 0).all()
        # without stats and without the optional count output: the same rows (query 8 is an ordinary one here)
        G, P = shapes[-1]
        got, log = collapse_on_device(index, ids, dists, counts, None, G, P, want_counts=False)
        n_calls += 1
        want = H.group_by_label(ids, dists, counts, labels, G, P)
        GC.assert_grouped_equal(got[:4] + (want[4],), want, "no stats, pool=%d" % pool)
        assert got[4] is None and got[5] is None
        # a handle on which no label was ever set: one group, label 0
        got, _ = collapse_on_device(unlabelled, ids, dists, counts, None, min(3, pool), pool)
        want = H.group_by_label(ids, dists, counts, None, min(3, pool), pool)
        GC.assert_grouped_equal(got, want, "no labels, pool=%d" % pool)
        assert (got[4] <= 1).all() and (got[2] == 0).all() and got[4][5] == 1 and got[3][5, 0] == pool
    assert index.stat("grouped_launches") == launches + n_calls and index.stat("grouped_calls") == 0


# ---- 2. the unfiltered search --------------------------------------------------------------------------------------------
def shape_for(pool):
    return min(pool, 12), 3


@pytest.mark.parametrize("pool", [10, 64, 200, 256])
@pytest.mark.parametrize("kind", KINDS, ids=["f32", "quant8"])
def test_unfiltered_is_the_collapse_of_search_batch(kind, pool):
    index, vs, lv, Q, _ = world(kind)
    G, P = shape_for(pool)
    cand = index.search_batch(Q, pool, 256)
    got = index.search_batch_grouped(Q, G, P, pool, 256)
    want = H.group_by_label(cand[0], cand[1], cand[2], world_labels(), G, P)
    GC.assert_grouped_equal(got, want, "kind %d pool %d" % (kind, pool))
    assert np.array_equal(got[5], cand[3]), "stats are the candidate call's"
    assert (cand[2] == pool).all() and (got[4] >= 1).all() and (got[4] <= G).all() and (got[4] == G).any()
    if pool >= 64:  # the hot label's group overflows per_group somewhere
        assert ((got[2] == 5) & (got[3] == P)).any()
    if kind == H.VEC_F32 and pool == 64:  # ... and once against the CPU oracle's search, collapsed the same way
        o_ids, o_d, o_c, o_s = oracle_from_product(index, vs, lv).search_batch(Q, pool, 256)
        GC.assert_grouped_equal(got, H.group_by_label(o_ids, o_d, o_c, world_labels(), G, P), "oracle")
        assert np.array_equal(got[5][:, :3], o_s.astype(np.int64)[:, :3])


# ---- 3. the filtered searches ----------------------------------------------------------------------------------------------
def filter_args(nq):
    """per query: a row of the set (or MASK_NONE) and a range -- one label (about 80 ids), the hot label, a wide range"""
    mo = (np.arange(nq) % 3).astype(np.uint32)
    mo[mo == 2] = MAX
    lo = np.where(np.arange(nq) % 4 == 0, 7, np.where(np.arange(nq) % 4 == 1, 5, 0)).astype(np.uint32)
    hi = np.where(np.arange(nq) % 4 == 0, 7, np.where(np.arange(nq) % 4 == 1, 5, 30)).astype(np.uint32)
    return mo, lo, hi


def candidates(index, Q, pool, ef, s, mo, lo, hi):
    if s is not None and lo is not None:
        return index.search_batch_filtered_set_range(Q, pool, ef, s, mo, lo, hi)
    if s is not None:
        return index.search_batch_filtered_set(Q, pool, ef, s, mo)
    if lo is not None:
        return index.search_batch_filtered_range(Q, pool, ef, lo, hi)
    return index.search_batch(Q, pool, ef)


FORMS = ["range", "set", "both", "none_rows"]


def form_args(form, s, nq):
    mo, lo, hi = filter_args(nq)
    if form == "range":
        return None, None, lo, hi
    if form == "set":
        return s, (mo % 2).astype(np.uint32), None, None  # (rows 0 and 1 only)
    if form == "both":
        return s, mo, lo, hi
    return s, np.full(nq, MAX, dtype=np.uint32), None, None  # every query HNSW_MASK_NONE


@pytest.mark.parametrize("exact_max", [65536, 300, -1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS, ids=["f32", "quant8"])
def test_filtered_is_the_collapse_of_the_candidate_call(kind, form, exact_max):
    index, _, _, Q, rows_b = world(kind)
    s = index.mask_set(rows_b)
    fs, mo, lo, hi = form_args(form, s, NQ)
    pool, G, P = 40, 6, 4
    index.set_option("filter_exact_max", exact_max)
    try:
        cand = candidates(index, Q, pool, 64, fs, mo, lo, hi)
        got = index.search_batch_grouped(Q, G, P, pool, 64, mask_set=fs, mask_of=mo, lo=lo, hi=hi)
    finally:
        index.set_option("filter_exact_max", 65536)
        s.close()
    want = H.group_by_label(cand[0], cand[1], cand[2], world_labels(), G, P)
    GC.assert_grouped_equal(got, want, "kind %d %s exact_max %d" % (kind, form, exact_max))
    assert np.array_equal(got[5], cand[3])
    if exact_max == 300 and form in ("range", "both"):  # the planner sent some groups down the exact path, some not
        assert len(set(cand[4].tolist())) > 1, set(cand[4].tolist())
    if lo is not None:  # every group's label lies in its query's range
        for q in range(NQ):
            assert ((got[2][q, :got[4][q]] >= lo[q]) & (got[2][q, :got[4][q]] <= hi[q])).all()


@pytest.mark.parametrize("kind", KINDS, ids=["f32", "quant8"])
def test_under_deletions(kind):
    index, _, _, Q, rows_b = world(kind)
    deleted = np.concatenate([np.arange(100, 500, 3), np.arange(1000, 1100)])
    mo, lo, hi = filter_args(NQ)
    pool, G, P = 40, 6, 4
    index.mark_deleted(deleted)
    try:
        for fs_lo_hi in ((None, None), (lo, hi)):
            cand = candidates(index, Q, pool, 64, None, None, *fs_lo_hi)
            got = index.search_batch_grouped(Q, G, P, pool, 64, lo=fs_lo_hi[0], hi=fs_lo_hi[1])
            GC.assert_grouped_equal(got, H.group_by_label(cand[0], cand[1], cand[2], world_labels(), G, P), "deleted")
            assert np.array_equal(got[5], cand[3])
            assert not np.isin(got[0][got[0] != MAX], deleted).any() and (got[4] > 0).all()
        with pytest.raises(H.HnswError) as e:  # the candidate call's limit while ids are deleted
            index.search_batch_grouped(Q, G, P, 65, 64)
        assert e.value.code == _lib.ERR_ARG
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_grouped(Q, G, P, 65, 65)  # nothing deleted: the unfiltered limits again
    assert (got[4] >= 1).all()


def raw_grouped(index, Q, G, P, pool, ef, lo, hi):
    nq = Q.shape[0]
    ids, dists = np.full((nq, G, P), 7, dtype=np.uint32), np.full((nq, G, P), 3.5, dtype=np.float32)
    lab, sz, cnt = np.full((nq, G), 7, dtype=np.uint32), np.full((nq, G), 7, dtype=np.uint32), np.full(nq, 9, dtype=np.uint32)
    stats = np.zeros((nq, 4), dtype=np.int32)
    p = lambda a, t=u32p: None if a is None else a.ctypes.data_as(t)
    rc = _lib.lib().hnsw_search_batch_grouped(index._h, p(Q, f32p), nq, G, P, pool, ef, None, None, p(lo), p(hi), p(ids),
                                              p(dists, f32p), p(lab), p(sz), p(cnt),
                                              C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)))
    return rc, (ids, dists, lab, sz, cnt, stats)


@pytest.mark.parametrize("ranged", [False, True], ids=["unfiltered", "range"])
def test_a_nan_query_fails_alone(ranged):
    index, _, _, Q, _ = world(H.VEC_F32)
    Q = Q[:24].copy()
    Q[9, 4] = np.nan
    clean = np.delete(np.arange(24), 9)
    _, lo, hi = filter_args(24)
    lo, hi = (lo, hi) if ranged else (None, None)
    pool, G, P = 40, 6, 4
    rc, got = raw_grouped(index, Q, G, P, pool, 64, lo, hi)
    assert rc == _lib.ERR_NAN_INPUT
    assert got[5][9, 3] == _lib.ERR_NAN_INPUT and got[4][9] == 0 and (got[0][9] == MAX).all() and np.isposinf(got[1][9]).all()
    assert (got[2][9] == 0).all() and (got[3][9] == 0).all()
    # every other row is filled in: what the call returns for the clean queries alone
    alone = index.search_batch_grouped(Q[clean], G, P, pool, 64, lo=None if lo is None else lo[clean],
                                       hi=None if hi is None else hi[clean])
    GC.assert_grouped_equal(tuple(a[clean] for a in got[:5]), alone, "nan, ranged=%s" % ranged)
    assert (got[5][clean, 3] == 0).all()


# ---- 4. label changes are seen -------------------------------------------------------------------------------------------
def test_label_changes_are_seen():
    index, _, _, Q, _ = world(H.VEC_QUANT8)
    pool, G, P = 64, 8, 3
    cand = index.search_batch(Q, pool, 128)
    first = index.search_batch_grouped(Q, G, P, pool, 128)
    GC.assert_grouped_equal(first, H.group_by_label(cand[0], cand[1], cand[2], world_labels(), G, P), "before")
    words = index.stat("label_words_uploaded")
    changed = world_labels()
    changed[::2] = 1000 + (np.arange(N)[::2] % 3)
    index.set_labels(changed)
    try:
        second = index.search_batch_grouped(Q, G, P, pool, 128)
        GC.assert_grouped_equal(second, H.group_by_label(cand[0], cand[1], cand[2], changed, G, P), "after")
        assert index.stat("label_words_uploaded") > words
        assert not np.array_equal(first[2], second[2]) and (second[2] >= 1000).any()
    finally:
        index.set_labels(world_labels())
    third = index.search_batch_grouped(Q, G, P, pool, 128)
    GC.assert_grouped_equal(third, first, "put back")


# ---- 5. launch accounting --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=["f32", "quant8"])
def test_an_unfiltered_call_is_the_search_plus_one_collapse(kind):
    index, _, _, Q, _ = world(kind)
    pool, G, P = 64, 8, 3
    index.search_batch_grouped(Q, G, P, pool, 128)  # (the label column is in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q, pool, 128)
    calls, launches = index.stat("grouped_calls"), index.stat("grouped_launches")
    with H.kernel_log() as log:
        index.search_batch_grouped(Q, G, P, pool, 128)
    assert log.get("hx_filt_merge_kernel") == 1, dict(log)
    assert "hx_filt_merge_kernel" not in plain and set(log) <= set(plain) | {"hx_filt_merge_kernel"}, (dict(log), dict(plain))
    assert index.stat("grouped_calls") == calls + 1 and index.stat("grouped_launches") == launches + 1
