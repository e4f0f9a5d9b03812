"""Hybrid search on the GPU (include/hnsw_mi355x.h, "hybrid search"), held to the numpy restatement of the rank fusion
(hnsw_rs_amd.hybrid.fuse_ranked; tests/test_hybrid_host.py holds that to a plain loop) over the CPU oracle's distances
(OracleHNSW.distance_batch) and search (OracleHNSW.search_batch).  All comparisons are exact: ids, score and distance
BITS, counts, unique, dropped, counters and statuses.
  1. hnsw_fuse_ranked_device alone over host-made lists at the pass boundaries of both vector kinds and the table's end,
     in both modes, with and without a dense list, E = 0 and E = 7: one launch and nothing else, guard words, no word
     unwritten, a bad id, a NaN query and a failed dense status failing their query alone;
  2. the same under deletions, a set row, a range, and both;
  3. search_batch_hybrid against the restatement over the ORACLE's lists, unfiltered and under a set row AND a range with
     ids deleted (the dense list of a filtered call on these small indexes is the exact path's: the nearest admissible
     ids by (distance bits, id), restated here over the oracle's distances);
  4. the entry point: a NaN query, the cosine option, launch accounting, a replica handle;
  5. capture and replay of the primitive and of the chain search -> fuse_ranked on a torch stream;
  6. a short random walk of inserts, deletions, relabelling and mask updates with one hybrid call after every step.
The indexes are those of tests/test_gpu_from_rows.py (built once, shared; what a test changes it puts back)."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import hybrid_cases as HC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import (M, N, SHAPES, capture_and_replay, guarded, kernel_of, unguard, up,  # noqa: F401
                                      world)
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
NQ = 64
POOL, TOPN, EF, EXT_W = 16, 10, 32, 12
# (chosen on the CPU: with these the oracle's lists meet HC.exercised on all four shapes, unfiltered and filtered)
QUERY_SEED, EXT_SEED, FILTER_SEED = 7, 23, 5
# candidate totals at the pass boundaries of both vector kinds (32 and 64 entries a pass) and at the table's end, as
# (dense pool or 0, external lists, their width): a dense list alone, no dense list, pool != width, E = 7
TOTALS = {1: (1, 0, 0), 31: (0, 1, 31), 32: (16, 2, 8), 33: (5, 7, 4), 63: (21, 2, 21), 64: (0, 4, 16), 65: (13, 4, 13),
          200: (100, 1, 100), 256: (64, 3, 64)}
NQ1 = 32  # queries of a host-made call


def dense_stats(stats_in, statuses):
    """the dense record as the fusion leaves it: its counters, the fusion's status"""
    s = np.asarray(stats_in).astype(np.int64).copy()
    s[:, 3] = np.asarray(statuses).astype(np.int64) & 0xFFFFFFFF
    return s


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def fuse_on_device(index, mode, rc, n_out, lists, w, ab, filt=None, mask_set=None, extras=True):
    """lists: (Q or None, ids0, counts0, stats0 [nq, 4], ext_ids, ext_scores, ext_counts) on the host; filt: naive's dict (its
    mask_of / lo / hi go to HBM; the deleted ids, the rows and the labels are the index's own state)"""
    import torch
    Q, ids0, c0, st0, ext, sc, ce = lists
    nq = ids0.shape[0] if ids0 is not None else ext.shape[0]
    E, W = (ext.shape[1], ext.shape[2]) if ext is not None else (0, 0)
    dev = lambda a: None if a is None else up(a)  # noqa: E731
    filt = filt or {}
    mo = None if filt.get("mask_of") is None else np.where(np.asarray(filt["mask_of"]) < 0, MAX, filt["mask_of"]).astype(np.uint32)
    d_in = [dev(x) for x in (ids0, c0, None if st0 is None else st0.astype(np.uint32), ext, sc, ce, w, Q, mo,
                             filt.get("lo"), filt.get("hi"))]
    sizes = {"ids": nq * n_out, "scores": nq * n_out, "dists": nq * n_out if (extras and Q is not None) else 0,
             "counts": nq if extras else 0, "unique": nq if extras else 0, "dropped": nq if extras else 0,
             "stats": 0 if st0 is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.fuse_ranked_device(nq, mode, rc, n_out, 0 if ids0 is None else ids0.shape[1], d_in[0], d_in[1], d_in[2], E, W,
                                 d_in[3], d_in[4], d_in[5], d_in[6], ab, d_in[7], out["ids"], out["scores"], out["dists"],
                                 out["counts"], out["unique"], out["dropped"], out["stats"], mask_set, d_in[8], d_in[9],
                                 d_in[10], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shape = (nq, n_out)
    return (got["ids"].reshape(shape), got["scores"].view(np.float32).reshape(shape),
            None if got["dists"] is None else got["dists"].view(np.float32).reshape(shape), got["counts"], got["unique"],
            got["dropped"], None if got["stats"] is None else got["stats"].reshape(nq, 4).astype(np.int64)), log


def host_made_lists(stored, p0, E, W, seed, nq=NQ1, legal=False):
    """nq queries: ids drawn where the index holds every row twice (0 .. 99 and 1400 .. 1499: equal distances, so LINEAR
    scores tie and the id decides) and anywhere, duplicates inside and across lists, ragged counts, a stats record for the
    dense list; external scores on a grid of quarters; rows near stored rows.  Planted: 0 no entry; 1 the lists identical;
    2 every entry distinct; 4 an id equal to the length; 5 a NaN in the row; 6 a failed dense status (legal: none of the
    last three).  -> (Q, ids0, counts0, stats0, ext_ids, ext_scores, ext_counts), weights [nq, 1 + E]"""
    rng = np.random.default_rng(seed)
    widths = ([p0] if p0 else []) + [W] * E
    total = sum(widths)
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    twins = np.concatenate([np.arange(100), np.arange(1400, 1500)])
    flat = np.where(rng.random((nq, total)) < 0.5, rng.choice(twins, (nq, total)), rng.integers(0, N, (nq, total))).astype(np.uint32)
    counts = np.stack([rng.integers(0, w + 1, nq) for w in widths], axis=1).astype(np.uint32)
    counts[::3] = widths
    counts[2] = np.array(widths) + 5
    counts[0] = 0
    one = rng.permutation(N)[:max(widths)].astype(np.uint32)
    for l, w in enumerate(widths):
        flat[1, starts[l]:starts[l] + w] = one[:w]
    counts[1] = widths
    flat[2] = rng.permutation(N)[:total]  # all distinct: `total` candidates, the kernel's last pass full
    stats = rng.integers(2 ** 31, 2 ** 32, (nq, 4)).astype(np.int64)
    stats[:, 3] = 0
    Q = stored[rng.integers(0, N, nq)] + rng.normal(0, 0.05, (nq, stored.shape[1])).astype(np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if not legal:
        flat[4, total - 1], counts[4] = N, widths
        Q[5, stored.shape[1] // 2] = np.nan
        stats[6, 3] = _lib.ERR_OVERFLOW & 0xFFFFFFFF
    w = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0, 1.0, 2.0], dtype=np.float32), (nq, 1 + E))
    ids0 = np.ascontiguousarray(flat[:, :p0]) if p0 else None
    ext = np.ascontiguousarray(flat[:, p0:].reshape(nq, E, W)) if E else None
    sc = (rng.integers(-8, 9, (nq, E, W)).astype(np.float32) * np.float32(0.25)) if E else None
    c0 = counts[:, 0].copy() if p0 else None
    ce = np.ascontiguousarray(counts[:, (1 if p0 else 0):]) if E else None
    return (Q, ids0, c0, stats if p0 else None, ext, sc, ce), np.ascontiguousarray(w)


def restated(mode, rc, n_out, lists, w, ab, orc, adm=None, n_points=N, with_q=True):
    Q, ids0, c0, st0, ext, sc, ce = lists
    statuses = None if st0 is None else st0[:, 3].astype(np.uint32).view(np.int32).astype(np.int64)
    return H.fuse_ranked(mode, rc, n_out, ids0, c0, statuses, ext, sc, ce, w, ab, Q if with_q else None, orc.distance_batch, adm,
                         n_points)


@pytest.mark.parametrize("total", list(TOTALS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_primitive_alone_is_the_restatement_bit_for_bit(name, total):
    index, orc, stored = world(name)
    index.upload()
    p0, E, W = TOTALS[total]
    assert p0 + E * W == total
    lists, w = host_made_lists(stored, p0, E, W, 100 * total + len(name))
    ab = None if E == 0 else (np.arange(E, dtype=np.float32) * np.float32(0.5) - np.float32(1.0))
    launches = index.stat("hybrid_fuse_launches")
    # with everything: weights, counts, stats, the query's row and every optional output
    for mode, rc, n_out in (("rrf", 60, min(10, total)), ("linear", 0, total), ("rrf", 1, total)):
        what = "%s total=%d mode=%s" % (name, total, mode)
        got, log = fuse_on_device(index, mode, rc, n_out, lists, w, ab)
        assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
        want = restated(mode, rc, n_out, lists, w, ab, orc)
        HC.assert_equal(got[:6], want, what)
        if p0:
            assert np.array_equal(got[6], dense_stats(lists[3], want[6])), what
        # a bad id, a NaN row and a failed status fail their query alone
        assert want[6][4] == _lib.ERR_ARG and want[6][5] == _lib.ERR_NAN_INPUT
        assert want[6][6] == (_lib.ERR_OVERFLOW if p0 else 0) and (want[6] != 0).sum() == (3 if p0 else 2)
        assert want[3][0] == 0 and want[4][2] == total and (want[5] == 0).all()
        for q in (4, 5) + ((6,) if p0 else ()):
            assert got[3][q] == 0 and got[4][q] == 0 and (got[0][q] == MAX).all() and np.isposinf(got[2][q]).all()
            assert (got[1][q] == (-np.inf if mode == "rrf" else np.inf)).all()
        assert (got[3][[3, 9]] >= 1).all()  # (every third query has full counts)
    # bare: no weights, no counts (pads mark the absent entries), no stats, no row, no optional output
    Q, ids0, c0, st0, ext, sc, ce = lists
    b0 = None if ids0 is None else ids0.copy()
    be = None if ext is None else ext.copy()
    if b0 is not None:
        b0[np.arange(p0)[None, :] >= c0[:, None]] = MAX
        b0[6] = MAX  # (without statuses query 6 cannot fail: it has no dense entry instead)
    if be is not None:
        be[np.arange(W)[None, None, :] >= ce[:, :, None]] = MAX
    bare = (None, b0, None, None, be, sc, None)
    for mode in ("rrf",) + (("linear",) if E else ()):
        got, log = fuse_on_device(index, mode, 60, min(10, total), bare, None, None, extras=False)
        want = restated(mode, 60, min(10, total), bare, None, None, orc, with_q=False)
        HC.assert_equal((got[0], got[1]), (want[0], want[1]), name + " bare " + mode)
        assert all(g is None for g in got[2:]) and dict(log) == {kernel_of(index): 1}
    assert index.stat("hybrid_fuse_launches") == launches + 3 + (2 if E else 1)


# ---- 2. the primitive under each filter kind ------------------------------------------------------------------------------
ALLOW_BITS = 1300  # the set's rows cover fewer ids than the index holds


class Filtered:
    """the shared index with ids deleted, labels set and a mask set, for the length of a `with`; everything is put back"""

    def __init__(self, index, kind, seed, nq):
        rng = np.random.default_rng(seed)
        self.index, self.kind, self.filt, self.set = index, kind, {}, None
        if kind in ("deleted", "both"):
            self.filt["deleted"] = np.sort(rng.permutation(N)[:N // 8]).astype(np.uint32)
        if kind in ("set", "both"):
            self.filt["masks"] = rng.random((3, ALLOW_BITS)) < 0.6
            mo = rng.integers(-1, 3, nq)
            mo[3] = 9  # a row the set does not have
            self.filt["mask_of"] = mo
        if kind in ("range", "both"):
            self.filt["labels"] = rng.integers(0, 6, N).astype(np.uint32)
            lo = rng.integers(0, 3, nq)
            hi = lo + rng.integers(0, 4, nq)
            lo[7], hi[7] = 3, 2  # lo > hi
            self.filt["lo"], self.filt["hi"] = lo.astype(np.uint32), hi.astype(np.uint32)

    def __enter__(self):
        self.labels_before = self.index.get_labels()
        if "deleted" in self.filt:
            self.index.mark_deleted(self.filt["deleted"])
        if "labels" in self.filt:
            self.index.set_labels(self.filt["labels"])
        if "masks" in self.filt:
            self.set = self.index.mask_set(self.filt["masks"], ALLOW_BITS)
        return self

    def __exit__(self, *exc):
        if self.set is not None:
            self.set.close()
        if "deleted" in self.filt:
            self.index.unmark_deleted(self.filt["deleted"])
        if "labels" in self.filt:
            self.index.set_labels(self.labels_before)

    def admissible(self, nq):
        return H.filters_of(nq, **HC.filters_args(self.filt))


@pytest.mark.parametrize("kind", ["deleted", "set", "range", "both"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_primitive_under_each_filter_kind(name, kind):
    index, orc, stored = world(name)
    index.upload()
    for total in (32, 65):
        p0, E, W = TOTALS[total]
        lists, w = host_made_lists(stored, p0, E, W, 7 * total + len(name) + len(kind))
        ab = np.full(E, 0.25, dtype=np.float32)
        with Filtered(index, kind, 11 * total + len(name), NQ1) as f:
            adm = f.admissible(NQ1)
            for mode, rc, n_out in (("rrf", 60, 10), ("linear", 0, total)):
                what = "%s %s total=%d mode=%s" % (name, kind, total, mode)
                got, log = fuse_on_device(index, mode, rc, n_out, lists, w, ab, f.filt, f.set)
                assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
                want = restated(mode, rc, n_out, lists, w, ab, orc, adm)
                HC.assert_equal(got[:6], want, what)
                assert np.array_equal(got[6], dense_stats(lists[3], want[6])), what
                assert want[5].sum() > 0, what + ": nothing was removed"
                if kind in ("set", "both"):
                    assert want[6][3] == _lib.ERR_ARG and got[3][3] == 0 and (f.filt["mask_of"] == -1).any()
                    beyond = np.concatenate([lists[0 + 1].reshape(-1), lists[4].reshape(-1)])
                    assert ((beyond >= ALLOW_BITS) & (beyond < N)).any(), "no id at or beyond allow_bits"
                if kind in ("range", "both"):
                    assert want[6][7] == 0 and want[4][7] == 0 and (want[5][7] > 0 or want[3][7] == 0)
                if "deleted" in f.filt:
                    assert not np.isin(got[0], f.filt["deleted"]).any()


# ---- 3. the search against the restatement over the oracle's lists --------------------------------------------------------
def near_queries(stored, nq, seed, noise=0.02):
    rng = np.random.default_rng(seed)
    q = stored[rng.choice(N, nq, replace=False)] + rng.normal(0, noise, (nq, stored.shape[1])).astype(np.float32)
    return np.ascontiguousarray(q, dtype=np.float32)


def external_lists(orc, Q, E, seed):
    """what another retriever might say: per list the oracle's search of a perturbed query mixed with random ids (a third
    of the entries), scores on a grid of quarters that fall with the position, ragged counts"""
    rng = np.random.default_rng(seed)
    nq = Q.shape[0]
    ext = np.zeros((nq, E, EXT_W), dtype=np.uint32)
    for e in range(E):
        P = (Q + rng.normal(0, 0.05, Q.shape)).astype(np.float32)
        found = np.asarray(orc.search_batch(P, EXT_W, EF)[0]).astype(np.uint32)
        mixed = np.where(rng.random((nq, EXT_W)) < 0.33, rng.integers(0, N, (nq, EXT_W)), found)
        ext[:, e] = mixed
    sc = (np.float32(4.0) - np.float32(0.25) * (np.arange(EXT_W) // 2).astype(np.float32))[None, None, :] * np.ones((nq, E, 1), np.float32)
    ce = rng.integers(EXT_W // 2, EXT_W + 1, (nq, E)).astype(np.uint32)
    return ext, np.ascontiguousarray(sc, dtype=np.float32), ce


def oracle_dense(orc, Q, pool, ef):
    c = orc.search_batch(Q, pool, ef)
    stats = np.concatenate([np.asarray(c[3]).astype(np.int64), np.zeros((Q.shape[0], 1), dtype=np.int64)], axis=1)
    return np.asarray(c[0]).astype(np.uint32), np.asarray(c[2]).astype(np.uint32), stats


def exact_dense(dist, Q, pool, adm, n_points):
    """the exact path of a filtered search on a small index: per query the `pool` nearest admissible ids by (distance bits,
    id), n_dist = the admissible ids, n_exp = sum_deg = 0"""
    nq = Q.shape[0]
    ids = np.full((nq, pool), MAX, dtype=np.uint32)
    counts, stats = np.zeros(nq, dtype=np.uint32), np.zeros((nq, 4), dtype=np.int64)
    every = np.arange(n_points, dtype=np.uint32)
    for q in range(nq):
        a = every[adm[q](every)]
        stats[q, 0] = a.size
        if a.size == 0:
            continue
        d = np.ascontiguousarray(dist(Q[q], a), dtype=np.float32)
        order = np.lexsort((a, d.view(np.uint32)))[:pool]
        ids[q, :order.size], counts[q] = a[order], order.size
    return ids, counts, stats


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_search_is_the_restatement_over_the_oracles_lists(name, E):
    index, orc, stored = world(name)
    Q = near_queries(stored, NQ, QUERY_SEED)
    ext, sc, ce = external_lists(orc, Q, E, EXT_SEED)
    ids0, c0, st0 = oracle_dense(orc, Q, POOL, EF)
    w = np.array([1.0] + [-0.5] * E, dtype=np.float32)
    plain = HC.naive(HC.RRF, 60, TOPN, ids0, c0, None, ext, sc, ce, None, None, None, None, None, N)
    ex = HC.exercised(ids0, c0, ext, ce, plain)
    assert ex["ext_only"], "no answer holds an id only an external list proposed"
    assert ex["both"], "no answer holds an id both proposed"
    assert ex["tie"], "no pair of returned hits ties on score"
    for mode, weights in (("rrf", None), ("rrf", w), ("linear", w), ("linear", None)):
        what = "%s E=%d mode=%s weights=%s" % (name, E, mode, weights is not None)
        wq = None if weights is None else np.tile(weights, (NQ, 1))
        want = H.fuse_ranked(mode, 60, TOPN, ids0, c0, None, ext, sc, ce, wq, None, Q, orc.distance_batch, None, N)
        got = index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, ce, mode=mode, weights=weights)
        HC.assert_equal(got[:6], want[:6], what)
        assert np.array_equal(got[6], dense_stats(st0, want[6])), what
        assert (got[3] == TOPN).all() and (got[5] == 0).all() and (got[6][:, 3] == 0).all()


@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_filtered_search_is_the_restatement_over_the_oracles_lists(name, E):
    index, orc, stored = world(name)
    Q = near_queries(stored, NQ, QUERY_SEED)
    ext, sc, ce = external_lists(orc, Q, E, EXT_SEED)
    with Filtered(index, "both", FILTER_SEED, NQ) as f:
        f.filt["mask_of"][3] = 1  # (a host call refuses a row the set does not have: every query names a real one or none)
        f.filt["lo"][7], f.filt["hi"][7] = 0, 5
        adm = f.admissible(NQ)
        ids0, c0, st0 = exact_dense(orc.distance_batch, Q, POOL, adm, N)
        removed = []
        plain = HC.naive(HC.RRF, 60, TOPN, ids0, c0, None, ext, sc, ce, None, None, None, None, f.filt, N, removed)
        ex = HC.exercised(ids0, c0, ext, ce, plain, removed, filtered=True)
        for key in ("ext_only", "both", "tie", "by_deleted", "by_mask", "by_label", "shifted"):
            assert ex[key], "the oracle's lists do not exercise: " + key
        for mode in ("rrf", "linear"):
            what = "%s E=%d filtered mode=%s" % (name, E, mode)
            want = H.fuse_ranked(mode, 60, TOPN, ids0, c0, None, ext, sc, ce, None, None, Q, orc.distance_batch, adm, N)
            HC.assert_equal(want, HC.naive(HC.RRF if mode == "rrf" else HC.LINEAR, 60, TOPN, ids0, c0, None, ext, sc, ce, None,
                                           None, Q, orc.distance_batch, f.filt, N), what + " (the two restatements)")
            got = index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, ce, mode=mode, mask_set=f.set,
                                            mask_of=f.filt["mask_of"], lo=f.filt["lo"], hi=f.filt["hi"])
            HC.assert_equal(got[:6], want[:6], what)
            assert np.array_equal(got[6], dense_stats(st0, want[6])), what
            assert (got[5] > 0).any() and not np.isin(got[0], f.filt["deleted"]).any()


# ---- 4. the entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-16", "quant8-40"])
def test_a_nan_query_fails_alone_with_the_query_named(name):
    index, orc, stored = world(name)
    Q = near_queries(stored, 16, 11)
    ext, sc, ce = external_lists(orc, Q, 1, 12)
    Q[3, 1] = np.nan
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ids, scores = np.full((16, TOPN), 7, dtype=np.uint32), np.full((16, TOPN), 3.5, dtype=np.float32)
    dists = np.full((16, TOPN), 3.5, dtype=np.float32)
    counts, unique, dropped = (np.full(16, 9, dtype=np.uint32) for _ in range(3))
    stats = np.zeros((16, 4), dtype=np.int32)
    L = _lib.lib()
    rc = L.hnsw_search_batch_hybrid(index._h, Q.ctypes.data_as(f32p), 16, TOPN, POOL, EF, 0, 60, 1, EXT_W, ext.ctypes.data_as(u32p),
                                    sc.ctypes.data_as(f32p), ce.ctypes.data_as(u32p), None, None, None, None, None, None,
                                    ids.ctypes.data_as(u32p), scores.ctypes.data_as(f32p), dists.ctypes.data_as(f32p),
                                    counts.ctypes.data_as(u32p), unique.ctypes.data_as(u32p), dropped.ctypes.data_as(u32p),
                                    C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)))
    assert rc == _lib.ERR_NAN_INPUT and L.hnsw_last_error().startswith(b"query 3:")
    assert counts[3] == 0 and unique[3] == 0 and dropped[3] == 0 and (ids[3] == MAX).all() and np.isneginf(scores[3]).all()
    assert np.isposinf(dists[3]).all() and stats[3, 3] == _lib.ERR_NAN_INPUT
    good = np.delete(np.arange(16), 3)  # every other row is filled in
    want = index.search_batch_hybrid(Q[good], TOPN, POOL, EF, ext[good], sc[good], ce[good])
    assert np.array_equal(ids[good], want[0]) and np.array_equal(scores[good].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(dists[good].view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(counts[good], want[3]) and np.array_equal(unique[good], want[4]) and (stats[good, 3] == 0).all()


@pytest.mark.parametrize("name", ["f32-16", "quant8-100"])
def test_a_call_is_one_search_and_one_fusion(name):
    index, orc, stored = world(name)
    Q = near_queries(stored, NQ, QUERY_SEED)
    ext, sc, ce = external_lists(orc, Q, 2, EXT_SEED)
    index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, ce)  # (the snapshot is in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q, POOL, EF)
    keys = ("hybrid_calls", "hybrid_fuse_launches", "uploads")
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, ce, mode="linear")
    fk = kernel_of(index)
    assert log.get(fk) == 1 and fk not in plain, (dict(log), dict(plain))
    assert {k: v for k, v in log.items() if k != fk} == dict(plain), (dict(log), dict(plain))  # one search, as the plain call
    assert {k: index.stat(k) for k in keys} == {"hybrid_calls": before["hybrid_calls"] + 1,
                                                "hybrid_fuse_launches": before["hybrid_fuse_launches"] + 1,
                                                "uploads": before["uploads"]}


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_cosine_option(kind):
    n, d = 1200, 24
    vs = (rand_vectors(n, d, 91) - np.float32(0.3)).astype(np.float32)
    lv = O.draw_levels(n, M, 9)
    index = H.HNSW.new(M, 32, d, kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=lv)
    # the oracle: a plain index over rows normalised beforehand by the option's arithmetic, asked with unit queries
    orc = oracle_from_product(index, SC.unit(vs), lv)
    rng = np.random.default_rng(17)
    Q = np.ascontiguousarray(vs[rng.choice(n, NQ, replace=False)] + rng.normal(0, 0.02, (NQ, d)).astype(np.float32), dtype=np.float32)
    Qu = SC.unit(Q)
    ids0, c0, st0 = oracle_dense(orc, Qu, POOL, EF)
    ext = rng.integers(0, n, (NQ, 1, EXT_W)).astype(np.uint32)
    ext[:, 0, ::2] = ids0[:, :EXT_W // 2]
    sc = rng.integers(0, 9, (NQ, 1, EXT_W)).astype(np.float32) * np.float32(0.25)
    w = np.array([1.0, 0.5], dtype=np.float32)
    for mode in ("rrf", "linear"):
        want = H.fuse_ranked(mode, 60, TOPN, ids0, c0, None, ext, sc, None, np.tile(w, (NQ, 1)), None, Qu, orc.distance_batch, None, n)
        got = index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, mode=mode, weights=w)
        HC.assert_equal(got[:6], want[:6], "cosine " + mode)
        assert np.array_equal(got[6], dense_stats(st0, want[6]))
        # the primitive makes its own unit copy of the caller's raw rows
        lists = (Q, ids0, c0, st0, ext, sc, None)
        got, log = fuse_on_device(index, mode, 60, TOPN, lists, np.tile(w, (NQ, 1)), None)
        HC.assert_equal(got[:6], want[:6], "cosine primitive " + mode)
        assert log.get(kernel_of(index)) == 1


def test_a_replica_handle_serves():
    import torch
    index, orc, stored = world("quant8-100")
    index.upload()
    L = _lib.lib()
    desc, there = _lib.SnapshotDesc(), _lib.SnapshotDesc()
    _lib.check(L.hnsw_snapshot_describe(index._h, C.byref(desc)))
    rep = H.HNSW.new(M, 32, index.dim, index.vec_kind)
    for i in range(7):
        there.bytes[i] = desc.bytes[i]
    for i in range(32):
        there.header[i] = desc.header[i]
    _lib.check(L.hnsw_snapshot_adopt(rep._h, C.byref(there)))

    class Mem:
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    for i in range(7):
        if desc.bytes[i]:
            a = torch.as_tensor(Mem(int(desc.ptr[i]), int(desc.bytes[i])), device="cuda:0")
            b = torch.as_tensor(Mem(int(there.ptr[i]), int(there.bytes[i])), device="cuda:0")
            b.copy_(a)
    torch.cuda.synchronize()
    _lib.check(L.hnsw_snapshot_commit(rep._h))
    p0, E, W = TOTALS[65]
    lists, w = host_made_lists(stored, p0, E, W, 5)
    for mode in ("rrf", "linear"):
        got, log = fuse_on_device(rep, mode, 60, 10, lists, w, None)
        HC.assert_equal(got[:6], restated(mode, 60, 10, lists, w, None, orc), "replica " + mode)
        assert dict(log) == {kernel_of(index): 1}


# ---- 5. capture and replay ------------------------------------------------------------------------------------------------
CAP = (16, 2, 12)


def cap_inputs(stored, seed):
    """every query legal and every weight finite (the replayed bytes are compared, statuses included)"""
    lists, w = host_made_lists(stored, *CAP, seed, nq=NQ, legal=True)
    return lists, w


@pytest.mark.parametrize("mode", ["rrf", "linear"])
@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_the_primitive_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name, mode):
    import torch
    index, orc, stored = world(name)
    index.upload()
    made = {"real": cap_inputs(stored, 31), "decoy": cap_inputs(stored, 32)}
    names = ("Q", "ids0", "c0", "st0", "ext", "sc", "ce")
    inputs = {k: (made["real"][0][j], made["decoy"][0][j]) for j, k in enumerate(names)}
    inputs["w"] = (made["real"][1], made["decoy"][1])
    shapes = {"ids": (NQ, TOPN), "scores": (NQ, TOPN), "dists": (NQ, TOPN), "counts": (NQ,), "unique": (NQ,), "dropped": (NQ,),
              "stats": (NQ, 4)}
    ab = np.array([0.5, -0.5], dtype=np.float32)

    def enqueue(i, o, stream):
        index.fuse_ranked_device(NQ, mode, 60, TOPN, CAP[0], i["ids0"], i["c0"], i["st0"], CAP[1], CAP[2], i["ext"], i["sc"],
                                 i["ce"], i["w"], ab, i["Q"], o["ids"], o["scores"], o["dists"], o["counts"], o["unique"],
                                 o["dropped"], o["stats"], stream=stream)

    def want(which):
        lists, w = made[which]
        f = restated(mode, 60, TOPN, lists, w, ab, orc)
        assert (f[6] == 0).all()
        return (f[0], f[1].view(np.uint32), f[2].view(np.uint32), f[3], f[4], f[5], dense_stats(lists[3], f[6]).astype(np.uint32))

    call = SC.Call(torch, "fuse_ranked", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    capture_and_replay(torch, call, want, {kernel_of(index): 1})


@pytest.mark.parametrize("name", ["f32-100", "quant8-100"])
def test_the_chain_search_fuse_ranked_is_two_nodes_and_replays_the_direct_calls_bytes(name):
    """inside the capture conditions of hnsw_search_batch_device (ef <= 256, nothing deleted, cosine off); both launches
    are enqueued on ONE stream, so the captured graph is one chain without parallel branches.  _finish synchronises and is
    no part of a captured graph: the direct chain is run with it as well, to the same bytes."""
    import torch
    index, orc, stored = world(name)
    index.upload()
    qs = {"real": near_queries(stored, NQ, 41), "decoy": near_queries(stored, NQ, 42)}
    exts = {k: external_lists(orc, qs[k], 1, 43) for k in qs}
    inputs = {"Q": (qs["real"], qs["decoy"]), "ext": (exts["real"][0], exts["decoy"][0]), "sc": (exts["real"][1], exts["decoy"][1]),
              "ce": (exts["real"][2], exts["decoy"][2])}
    shapes = {"ids": (NQ, TOPN), "scores": (NQ, TOPN), "dists": (NQ, TOPN), "counts": (NQ,), "unique": (NQ,), "dropped": (NQ,),
              "stats": (NQ, 4)}
    dev = torch.device("cuda:0")
    mid = {"ids": torch.zeros((NQ, POOL), dtype=torch.int32, device=dev),
           "dists": torch.zeros((NQ, POOL), dtype=torch.int32, device=dev),
           "counts": torch.zeros(NQ, dtype=torch.int32, device=dev),
           "stats": torch.zeros((NQ, 4), dtype=torch.int32, device=dev)}

    def search_args(i, stream):
        return (i["Q"].data_ptr(), NQ, POOL, EF, mid["ids"].data_ptr(), mid["dists"].data_ptr(), mid["counts"].data_ptr(),
                mid["stats"].data_ptr(), stream)

    def enqueue(i, o, stream, finish=False):
        index.search_batch_device(*search_args(i, stream))
        if finish:
            index.search_batch_device_finish(*search_args(i, stream))
        index.fuse_ranked_device(NQ, "linear", 0, TOPN, POOL, mid["ids"], mid["counts"], mid["stats"], 1, EXT_W, i["ext"], i["sc"],
                                 i["ce"], None, None, i["Q"], o["ids"], o["scores"], o["dists"], o["counts"], o["unique"],
                                 o["dropped"], o["stats"], stream=stream)

    def want(which):
        ids0, c0, st0 = oracle_dense(orc, qs[which], POOL, EF)
        ext, sc, ce = exts[which]
        f = H.fuse_ranked("linear", 0, TOPN, ids0, c0, None, ext, sc, ce, None, None, qs[which], orc.distance_batch, None, N)
        return (f[0], f[1].view(np.uint32), f[2].view(np.uint32), f[3], f[4], f[5], dense_stats(st0, f[6]).astype(np.uint32))

    call = SC.Call(torch, "chain", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    # the direct chain with _finish in it
    call.load("real")
    call.poison()
    enqueue(call.inp, call.out, torch.cuda.current_stream().cuda_stream, finish=True)
    torch.cuda.synchronize()
    assert SC.verdict(call.arrays(copies=False), want("real")) is None
    with H.kernel_log() as plain:
        index.search_batch_device(*search_args(call.inp, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert sum(plain.values()) == 1, dict(plain)
    expected = dict(plain)
    expected[kernel_of(index)] = 1
    capture_and_replay(torch, call, want, expected)


# ---- 6. under updates -----------------------------------------------------------------------------------------------------
WALK_N, WALK_D, WALK_STEPS, WALK_BITS, WALK_NQ = 400, 16, 40, 480, 8


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_a_random_walk_of_updates_with_a_hybrid_call_after_every_step(kind):
    """insert_vec, mark / unmark_deleted, set_labels and mask_set.update interleaved at random; after each step one hybrid
    call under the set AND a range, with fixed external lists, equals the restatement over an oracle that holds the same
    points (the dense list of these calls is the exact path's: it needs the oracle's distances, not its graph)"""
    rng = np.random.default_rng(1234 + kind)
    vs = rand_vectors(WALK_N + WALK_STEPS, WALK_D, 77)
    lv = O.draw_levels(WALK_N + WALK_STEPS, M, 78)
    index = H.HNSW.new(M, 32, WALK_D, kind).insert_bulk(vs[:WALK_N], 2, False, levels=lv[:WALK_N])
    orc = O.OracleHNSW(M, 32, WALK_D, kind)
    orc.import_points(vs[:WALK_N], lv[:WALK_N])
    n = WALK_N
    deleted, labels = set(), np.zeros(WALK_N + WALK_STEPS, dtype=np.uint32)
    masks = rng.random((2, WALK_BITS)) < 0.7
    mset = index.mask_set(masks, WALK_BITS)
    Q = np.ascontiguousarray(vs[rng.choice(WALK_N, WALK_NQ, replace=False)] + np.float32(0.01), dtype=np.float32)
    ext = rng.integers(0, WALK_N, (WALK_NQ, 1, EXT_W)).astype(np.uint32)
    sc = rng.integers(0, 9, (WALK_NQ, 1, EXT_W)).astype(np.float32) * np.float32(0.25)
    mo = np.array([0, 1, -1, 0, 1, 0, -1, 1])
    lo, hi = np.array([0, 0, 1, 2, 0, 1, 0, 3], dtype=np.uint32), np.array([3, 1, 4, 2, 5, 3, 0, 2], dtype=np.uint32)
    seen = set()
    for step in range(WALK_STEPS):
        op = ("insert", "mark", "unmark", "labels", "mask")[int(rng.integers(0, 5))] if step >= 5 else \
            ("mark", "labels", "mask", "insert", "unmark")[step]
        seen.add(op)
        if op == "insert":
            assert index.insert_vec(vs[n], level=int(lv[n])) == n
            n += 1
            orc = O.OracleHNSW(M, 32, WALK_D, kind)  # (rebuilt alongside: the same points, no graph)
            orc.import_points(vs[:n], lv[:n])
        elif op == "mark":
            ids = rng.choice(n, 12, replace=False).astype(np.uint32)
            ids[:4] = ext[rng.integers(0, WALK_NQ, 4), 0, rng.integers(0, EXT_W, 4)]  # (what the external lists name)
            ids = np.unique(ids)
            index.mark_deleted(ids)
            deleted |= set(ids.tolist())
        elif op == "unmark":
            ids = np.array(sorted(deleted))[::2].astype(np.uint32)
            if ids.size:
                index.unmark_deleted(ids)
                deleted -= set(ids.tolist())
        elif op == "labels":
            ids = rng.choice(n, 60, replace=False).astype(np.uint32)
            vals = rng.integers(0, 6, 60).astype(np.uint32)
            index.set_labels(vals, ids)
            labels[ids] = vals
        else:
            row, ids, allow = int(rng.integers(0, 2)), rng.choice(WALK_BITS, 40, replace=False).astype(np.uint32), bool(rng.integers(0, 2))
            mset.update(row, ids, allow)
            masks[row, ids] = allow
        filt = dict(deleted=np.array(sorted(deleted), dtype=np.uint32), masks=masks, mask_of=mo, labels=labels[:n], lo=lo, hi=hi)
        adm = H.filters_of(WALK_NQ, **HC.filters_args(filt))
        ids0, c0, st0 = exact_dense(orc.distance_batch, Q, POOL, adm, n)
        mode = ("rrf", "linear")[step % 2]
        want = H.fuse_ranked(mode, 60, TOPN, ids0, c0, None, ext, sc, None, None, None, Q, orc.distance_batch, adm, n)
        got = index.search_batch_hybrid(Q, TOPN, POOL, EF, ext, sc, mode=mode, mask_set=mset, mask_of=mo, lo=lo, hi=hi)
        HC.assert_equal(got[:6], want[:6], "step %d (%s) mode=%s" % (step, op, mode))
        assert np.array_equal(got[6], dense_stats(st0, want[6])), "step %d (%s): the dense call's stats" % (step, op)
    assert seen == {"insert", "mark", "unmark", "labels", "mask"} and n > WALK_N
    mset.close()
