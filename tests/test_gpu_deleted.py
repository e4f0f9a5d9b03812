"""Deletion on the MI355X (include/hnsw_mi355x.h, "deletion"): every search entry point under deleted ids against the
CPU restatement of filtered search (tests/filtered_restate.py) with allowed = "not deleted", on a restatement of the
product's own graph -- ids, distance bits, counts, counters (n_dist, n_exp, sum_deg) and the path, read from the
deleted_* counters -- and against the filtered entry point on an undeleted clone."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from oracle import restate_np as R
from tests import filtered_restate as FR
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

LIMIT = 24576  # ids the largest visited table holds (32768 slots, 75 %)
DEL_KEYS = ("deleted_queries_graph", "deleted_queries_exact", "deleted_overflow_exact")


def restated(index, vectors):
    layers = [index.get_layer(l).csr() for l in range(index.nb_layers())]
    return R.Index.from_csr(vectors, index.vec_kind, layers, int(index.params.ep))


def counters(index, keys=DEL_KEYS):
    return np.array([index.stat(k) for k in keys], dtype=np.int64)


def restate(ridx, Qr, n, ef, deleted, n_points, exact_max):
    """-> per query (want, path or None when the restatement cannot tell 0 from 2)"""
    dead = set(int(i) for i in deleted)
    live = np.array([i for i in range(n_points) if i not in dead], dtype=np.int64)
    out = []
    for q in Qr:
        if live.size <= exact_max:
            out.append((FR.exact(ridx, q, n, live), 1))
            continue
        g = FR.graph(ridx, q, n, ef, lambda i: i not in dead)
        if g["visited0"] > LIMIT:
            out.append((FR.exact(ridx, q, n, live), 2))
        elif g["visited0"] + g["maxdeg0"] <= LIMIT:
            out.append((g, 0))
        else:
            out.append(((g, FR.exact(ridx, q, n, live)), None))
    return out


def compare(ids, dists, counts, stats, wants, n, what):
    """-> the paths taken (ambiguous queries resolved by which restatement the product matched)"""
    paths = []
    for qi, (want, path) in enumerate(wants):
        cands = [(want, path)] if path is not None else [(want[0], 0), (want[1], 2)]
        ok = None
        for w, p in cands:
            w_ids, w_d, w_c = FR.padded(w, n)
            if (counts[qi] == w_c and np.array_equal(ids[qi], w_ids)
                    and np.array_equal(dists[qi].view(np.uint32), w_d.view(np.uint32))
                    and tuple(int(x) for x in stats[qi, :3]) == tuple(w["counters"])):
                ok = p
                break
        assert ok is not None, (what, qi, ids[qi], FR.padded(cands[0][0], n)[0], stats[qi], cands[0][0]["counters"])
        paths.append(ok)
    return np.array(paths)


def check_batch(index, ridx, Q, n, ef, deleted, exact_max=-1, Qr=None, what=""):
    """search_batch with `deleted` marked against the restatement; the deleted_* counters must follow the paths"""
    Qr = Q if Qr is None else Qr
    index.set_option("filter_exact_max", exact_max)
    c0 = counters(index)
    ids, dists, counts, stats = index.search_batch(Q, n, ef)
    wants = restate(ridx, Qr, n, ef, deleted, index.len(), exact_max)
    paths = compare(ids, dists, counts, stats, wants, n, what)
    assert (stats[:, 3] == 0).all()
    assert not np.isin(ids, np.asarray(list(deleted), dtype=np.uint32)).any(), what
    dc = counters(index) - c0
    assert tuple(dc) == (int((paths == 0).sum()), int((paths == 1).sum()), int((paths == 2).sum())), (what, dc)
    return paths


def patterns(n_points, ep, seed):
    rng = np.random.default_rng(seed)
    out = [("one", [int(rng.integers(n_points))]), ("ep", [ep])]
    for frac in (0.01, 0.1, 0.5):
        out.append((str(frac), np.flatnonzero(rng.random(n_points) < frac).tolist()))
    return out


def build(kind, d, n=3000, seed=0, cosine=False):
    vs = rand_vectors(n, d, 40 + d + seed)
    if cosine:
        vs = vs - np.float32(0.5)
    index = H.HNSW.new(16, 64, d, kind)
    if cosine:
        index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=O.draw_levels(n, 16, 2 + seed))
    return index, vs


def unit(x):
    s = np.zeros(x.shape[0], dtype=np.float32)
    for e in range(x.shape[1]):
        s = s + x[:, e] * x[:, e]
    return x / np.sqrt(s)[:, None]


@pytest.mark.parametrize("kind,d,cosine", [(H.VEC_F32, 100, False), (H.VEC_F32, 128, False), (H.VEC_QUANT8, 100, False),
                                           (H.VEC_F32, 37, False), (H.VEC_QUANT8, 37, False), (H.VEC_F32, 32, True)],
                         ids=["f32-100", "f32-128", "q8-100", "f32-37", "q8-37", "cosine-32"])
def test_search_batch_under_deletions(kind, d, cosine):
    index, vs = build(kind, d, cosine=cosine)
    stored = np.stack([index.get_point(i).get_vals() for i in range(index.len())]) if cosine else vs
    ridx = restated(index, stored)
    qs = rand_vectors(24, d, 41 + d)
    if cosine:
        qs = qs - np.float32(0.5)
    Qr = unit(qs) if cosine else qs
    ep = int(index.params.ep)
    plain = index.search_batch(qs, 10, 64)
    launched = set()
    for name, dead in patterns(index.len(), ep, d):
        index.mark_deleted(dead)
        for n, ef in ((10, 64), (64, 128), (10, 5)):
            with H.kernel_log() as log:
                paths = check_batch(index, ridx, qs, n, ef, dead, Qr=Qr, what="%s n=%d ef=%d" % (name, n, ef))
            assert (paths == 0).all()
            launched |= set(log)
        index.unmark_deleted(dead)
    # once the mask is on the device, a search after (un)marking sends the touched words through the scatter kernel
    assert "hx_deleted_scatter_kernel" in launched, launched
    # all but a handful: the exact path at the default filter_exact_max
    keep = [7, 1500, 2999, 640, 12]
    dead = [i for i in range(index.len()) if i not in keep]
    index.mark_deleted(dead)
    paths = check_batch(index, ridx, qs, 10, 64, dead, exact_max=65536, Qr=Qr, what="handful")
    assert (paths == 1).all()
    # everything: count 0 on both paths
    index.mark_deleted(keep)
    for em in (-1, 65536):
        index.set_option("filter_exact_max", em)
        ids, dists, counts, stats = index.search_batch(qs, 10, 64)
        assert (counts == 0).all() and (ids == _lib.UINT32_MAX).all() and np.isinf(dists).all()
    # after unmarking everything: the never-deleted results, and the deleted_* counters stand still
    index.unmark_deleted(np.arange(index.len()))
    assert index.deleted_count() == 0
    c0 = counters(index)
    again = index.search_batch(qs, 10, 64)
    for a, b in zip(plain, again):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    assert (counters(index) == c0).all()


@pytest.fixture(scope="module")
def f32_100():
    index, vs = build(H.VEC_F32, 100, n=4000, seed=3)
    return index, vs, restated(index, vs), rand_vectors(40, 100, 77)


def test_equals_filtered_search_on_an_undeleted_clone(f32_100):
    index, vs, ridx, qs = f32_100
    rng = np.random.default_rng(11)
    dead = np.flatnonzero(rng.random(index.len()) < 0.2)
    clone = index.clone()
    index.mark_deleted(dead)
    try:
        for em in (-1, 65536):
            index.set_option("filter_exact_max", em)
            clone.set_option("filter_exact_max", em)
            live = np.ones(index.len(), dtype=bool)
            live[dead] = False
            for n, ef in ((10, 64), (64, 256), (1, 1)):
                a = index.search_batch(qs, n, ef)
                f0 = counters(clone, ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact"))
                b = clone.search_batch_filtered(qs, n, ef, live)
                for x, y in zip(a, b[:4]):
                    assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)), (em, n, ef)
                assert clone.stat("filtered_queries_exact" if em > 0 else "filtered_queries_graph") == \
                    f0[1 if em > 0 else 0] + qs.shape[0]
            # a filtered call under deletions: mask AND NOT deleted
            mask = rng.random(index.len()) < 0.5
            for n, ef in ((10, 64), (20, 30)):
                a = index.search_batch_filtered(qs, n, ef, mask)
                b = clone.search_batch_filtered(qs, n, ef, mask & live)
                for x, y in zip(a, b):
                    assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)), (em, n, ef)
            assert clone.deleted_count() == 0
    finally:
        index.unmark_deleted(dead)


def test_deleting_unvisited_ids_changes_nothing():
    """two components, the entry point's and one no walk reaches: deleting the second's ids leaves the unfiltered
    results and counters exactly as they were (ef >= n)"""
    n, d = 2000, 24
    vs = rand_vectors(n, d, 121)
    rng = np.random.default_rng(122)
    rows = [set() for _ in range(n)]
    half = n // 2
    for i in range(n):
        lo, hi = (0, half) if i < half else (half, n)
        for j in rng.integers(lo, hi, size=6).tolist():
            if j != i:
                rows[i].add(j)
                rows[j].add(i)
    index = _import_graph(vs, H.VEC_F32, 8, rows)
    qs = rand_vectors(30, d, 123)
    dead = np.arange(half, n, 3)
    for n_, ef in ((10, 10), (10, 64), (32, 200)):
        want = index.search_batch(qs, n_, ef)
        index.mark_deleted(dead)
        index.set_option("filter_exact_max", -1)
        got = index.search_batch(qs, n_, ef)
        index.unmark_deleted(dead)
        for a, b in zip(want, got):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (n_, ef)


def _import_graph(vs, kind, m, rows):
    n, d = vs.shape
    index = H.HNSW.new(m, None, d, kind)
    index.import_points(vs, np.zeros(n, dtype=np.uint8))
    flat = np.concatenate([np.array(sorted(r), dtype=np.uint32) for r in rows])
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    index.import_layer(0, np.arange(n, dtype=np.uint32), offs, flat)
    index.set_ep(0)
    return index


@pytest.fixture(scope="module")
def dense40k():
    """a dense random graph over 40000 points: with 99.9 % of the ids deleted R never fills, the walk visits every node
    and fills the largest visited table (path 2)"""
    n, d = 40000, 8
    vs = rand_vectors(n, d, 81)
    rng = np.random.default_rng(82)
    nbrs = rng.integers(0, n, size=(n, 10))
    rows = [set() for _ in range(n)]
    for i in range(n):
        for j in nbrs[i].tolist():
            if j != i:
                rows[i].add(j)
                rows[j].add(i)
    index = _import_graph(vs, H.VEC_F32, 8, rows)
    dead = np.flatnonzero(rng.random(n) >= 0.001)
    return index, vs, restated(index, vs), rand_vectors(3, d, 83), dead


def test_overflow_takes_the_exact_path(dense40k):
    index, vs, ridx, qs, dead = dense40k
    index.mark_deleted(dead)
    try:
        paths = check_batch(index, ridx, qs, 10, 64, dead, what="path 2")
        assert (paths == 2).all()
    finally:
        index.unmark_deleted(dead)


def test_device_form_equals_the_host_form(dense40k, f32_100):
    import torch
    dev = torch.device("cuda:0")
    for index, qs, dead in ((dense40k[0], dense40k[3], dense40k[4]),
                            (f32_100[0], f32_100[3], np.arange(0, f32_100[0].len(), 7))):
        index.mark_deleted(dead)
        try:
            index.set_option("filter_exact_max", -1)
            for n, ef in ((10, 64), (5, 3)):
                want = index.search_batch(qs, n, ef)
                c0 = counters(index)
                nq = qs.shape[0]
                dQ = torch.from_numpy(qs).to(dev)
                d_ids = torch.empty((nq, n), dtype=torch.int32, device=dev)
                d_d = torch.empty((nq, n), dtype=torch.float32, device=dev)
                d_c = torch.empty(nq, dtype=torch.int32, device=dev)
                d_s = torch.empty((nq, 4), dtype=torch.int32, device=dev)
                index.search_batch_device(dQ.data_ptr(), nq, n, ef, d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(),
                                          d_s.data_ptr(), 0)
                index.search_batch_device_finish(dQ.data_ptr(), nq, n, ef, d_ids.data_ptr(), d_d.data_ptr(),
                                                 d_c.data_ptr(), d_s.data_ptr(), 0)
                got = (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                       d_s.cpu().numpy().view(np.uint32).astype(np.int64))
                for a, b in zip(want, got):
                    assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (n, ef)
                dc = counters(index) - c0  # the host call counted its own; the device form counts the same again
                assert dc[1] == 0 and dc[0] + dc[2] == nq
                # without the optional outputs
                d_ids.fill_(0)
                index.search_batch_device(dQ.data_ptr(), nq, n, ef, d_ids.data_ptr(), 0, 0, d_s.data_ptr(), 0)
                index.search_batch_device_finish(dQ.data_ptr(), nq, n, ef, d_ids.data_ptr(), 0, 0, d_s.data_ptr(), 0)
                assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), want[0])
        finally:
            index.unmark_deleted(dead)


def test_one_query_calls_are_coalesced_under_deletions(f32_100):
    index = f32_100[0]
    qs = rand_vectors(128, 100, 78)  # (a thread per query at most: 64 threads need 64 queries)
    dead = np.arange(1, index.len(), 5)
    index.mark_deleted(dead)
    try:
        index.set_option("filter_exact_max", -1)
        want_ids, _, want_c, _ = index.search_batch(qs, 10, 64)
        q0, b0 = index.stat("coalesced_queries"), index.stat("coalesced_batches")
        g0 = index.stat("deleted_queries_graph")
        ids, counts, calls, wall, lat = index.search_threads(qs, 10, 64, 64, 1.5)
        assert calls > 0
        assert np.array_equal(ids, want_ids) and np.array_equal(counts, want_c)
        assert index.stat("coalesced_queries") - q0 == calls
        assert index.stat("coalesced_batches") - b0 < calls  # batches of more than one query
        assert index.stat("deleted_queries_graph") - g0 == calls
        # the one-query entry of the reference's API
        assert index.ann_by_vector(qs[3], 10, 64) == [int(x) for x in want_ids[3][: want_c[3]]]
    finally:
        index.unmark_deleted(dead)


def test_brute_force_excludes_deleted_ids(f32_100):
    index, vs, ridx, qs = f32_100
    want_plain = index.brute_force(qs, 10)
    dead = np.flatnonzero(np.random.default_rng(5).random(index.len()) < 0.3)
    index.mark_deleted(dead)
    try:
        ids, dists = index.brute_force(qs, 10)
        live = np.setdiff1d(np.arange(index.len()), dead)
        for qi in range(qs.shape[0]):
            w = FR.exact(ridx, qs[qi], 10, live)
            assert np.array_equal(ids[qi], w["ids"]) and np.array_equal(dists[qi].view(np.uint32), w["dists"].view(np.uint32))
        with pytest.raises(H.HnswError) as e:
            index.brute_force_fast(qs, 10)
        assert e.value.code == _lib.ERR_ARG
        index.mark_deleted(np.arange(index.len() - 3))
        ids, dists = index.brute_force(qs[:2], 10)  # three live ids, padding beyond
        assert (ids[:, 3:] == _lib.UINT32_MAX).all() and np.isinf(dists[:, 3:]).all()
        assert set(ids[0, :3].tolist()) == set(range(index.len() - 3, index.len()))
    finally:
        index.unmark_deleted(np.arange(index.len()))
    assert all(np.array_equal(a, b) for a, b in zip(want_plain, index.brute_force(qs, 10)))
    index.brute_force_fast(qs, 10)


def test_insert_vec_after_deletions_and_the_mask_upload():
    d = 24
    vs = rand_vectors(6400, d, 61)
    index = H.HNSW.new(8, 32, d, H.VEC_F32).insert_bulk(vs, 4, False, levels=O.draw_levels(6400, 8, 3))
    qs = rand_vectors(20, d, 63)
    index.mark_deleted(np.arange(0, 6400, 2))
    index.set_option("filter_exact_max", -1)
    index.search_batch(qs, 10, 64)  # uploads the snapshot and the whole mask (100 words)
    up, w0 = index.stat("uploads"), index.stat("deleted_mask_words_uploaded")
    assert up >= 1 and w0 == 100
    # a mark after an upload: only the touched words travel, the snapshot stays
    index.mark_deleted([1, 3, 65, 6399, 6397])  # words 0, 1, 99
    index.search_batch(qs, 10, 64)
    assert index.stat("deleted_mask_words_uploaded") == w0 + 3 and index.stat("uploads") == up
    index.mark_deleted([1])  # nothing changes: nothing travels
    index.search_batch(qs, 10, 64)
    assert index.stat("deleted_mask_words_uploaded") == w0 + 3
    # a new point is live and found, through the patched snapshot
    new = rand_vectors(1, d, 64)[0]
    nid = index.insert_vec(new)
    assert nid == 6400 and index.stat("uploads") == up and index.stat("point_patches") == 1
    ids, _, counts, _ = index.search_batch(new[None, :], 10, 64)
    assert ids[0, 0] == nid
    dead = set(index.deleted_ids().tolist())
    ids, _, counts, _ = index.search_batch(qs, 10, 64)
    assert not any(int(x) in dead for x in ids.reshape(-1))
    ridx = restated(index, np.concatenate([vs, new[None, :]]))
    check_batch(index, ridx, qs, 10, 64, sorted(dead), what="after insert_vec")
    assert index.stat("uploads") == up


def test_limits_apply_only_while_ids_are_deleted(f32_100):
    index, vs, ridx, qs = f32_100
    index.set_option("filter_exact_max", -1)
    for n, ef in ((65, 100), (10, 257), (300, 10)):
        index.search_batch(qs[:2], n, ef)
    index.mark_deleted([5])
    try:
        for n, ef in ((65, 100), (10, 257), (300, 10)):
            with pytest.raises(H.HnswError) as e:
                index.search_batch(qs[:2], n, ef)
            assert e.value.code == _lib.ERR_ARG, (n, ef)
        index.set_option("filter_exact_max", 65536)  # the exact path has no ef limit
        ids, _, counts, _ = index.search_batch(qs[:2], 10, 300)
        assert (counts == 10).all()
        # ef < n: up to n ids under deletions (the filtered contract)
        ids, _, counts, _ = index.search_batch(qs[:2], 20, 5)
        assert (counts == 20).all()
    finally:
        index.unmark_deleted([5])
    ids, _, counts, _ = index.search_batch(qs[:2], 20, 5)
    assert (counts == 5).all()
