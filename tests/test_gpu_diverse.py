"""Diversified search on the GPU (include/hnsw_mi355x.h, "diversified search"), held to the numpy restatement of the
selection (hnsw_rs_amd.diverse.mmr_select; tests/test_diverse_host.py holds that to a plain loop) with the CPU oracle's
pair distance.  All comparisons are exact: ids, distance BITS, gap BITS, counts and statuses.
  1. hnsw_diversify_device alone over synthetic device lists (no search), the host test's sweep, on four small indexes
     that hold 100 rows twice; ids beyond the index; one launch and nothing else; guard words behind every output;
  2. hnsw_search_batch_diverse against mmr_select over the ORACLE's search_batch and distance, on clustered rows;
  3. launch accounting, deletions, a label range and a mask-set row, the cosine option, the stat keys;
  4. capture and replay of the primitive on a torch stream."""
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import diverse_cases as DC
from tests import stream_cases as SC
from tests.util import oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A  # (as a float 1.5e16, as an id beyond every index here)
GUARD = 64  # words behind every output that no launch may write
N_SMALL, M = 1500, 16
SMALL = {"f32-16": (H.VEC_F32, 16), "f32-100": (H.VEC_F32, 100), "quant8-40": (H.VEC_QUANT8, 40),
         "quant8-100": (H.VEC_QUANT8, 100)}


def kernel_of(index):
    return "hx_distance_kernel<%d>" % index.vec_kind


@functools.lru_cache(maxsize=None)
def small_world(name):
    """an index of 1500 points whose rows 100 .. 199 repeat rows 0 .. 99 (pair distances of exactly 0, score ties), its
    snapshot in HBM, and the oracle's distances between the ids the synthetic lists use"""
    kind, d = SMALL[name]
    vs = rand_vectors(N_SMALL, d, 51 + d)
    vs[100:200] = vs[0:100]
    lv = O.draw_levels(N_SMALL, M, 51)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(vs, 4, False, levels=lv)
    index.upload()
    orc = oracle_from_product(index, vs, lv)
    pair = np.array([[orc.distance(a, b) for b in range(DC.ID_SPAN)] for a in range(DC.ID_SPAN)], dtype=np.float32)
    assert (np.diagonal(pair[:100, 100:200]) == 0).all()
    pair.setflags(write=False)
    return index, pair


def up(a):  # (uint32 travels as int32: the bits are what the kernel reads)
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).copy()).to(torch.device("cuda:0"))


def select_on_device(index, ids, dists, counts, stats, n_out, lam, want_gaps=True, want_counts=True):
    """hnsw_diversify_device over uploaded lists, every output followed by GUARD sentinel words
    -> (ids, dists, gaps or None, counts or None, stats or None), the kernel log"""
    import torch
    dev = torch.device("cuda:0")
    nq, pool = ids.shape
    d_in = (up(ids), up(dists), None if counts is None else up(counts),
            None if stats is None else up(stats.astype(np.uint32)))
    sizes = {"ids": nq * n_out, "dists": nq * n_out, "gaps": nq * n_out if want_gaps else 0,
             "counts": nq if want_counts else 0, "stats": 0 if stats is None else nq * 4}
    out = {k: torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev) if n else None for k, n in sizes.items()}
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        index.diversify_device(nq, pool, n_out, lam, d_in[0], d_in[1], d_in[2], d_in[3], out["ids"], out["dists"],
                               out["gaps"], out["counts"], out["stats"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = {}
    for k, t in out.items():
        if t is None:
            got[k] = None
            continue
        a = t.cpu().numpy().view(np.uint32)
        assert (a[sizes[k]:] == SENTINEL).all(), "%s: a guard word behind the output was written" % k
        assert not (a[:sizes[k]] == SENTINEL).any(), "%s: an output word was left unwritten" % k
        got[k] = a[:sizes[k]]
    shape = (nq, n_out)
    return (got["ids"].reshape(shape), got["dists"].view(np.float32).reshape(shape),
            None if got["gaps"] is None else got["gaps"].view(np.float32).reshape(shape), got["counts"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4).view(np.int32).astype(np.int64)), log


# ---- 1. the primitive alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", DC.POOLS)
@pytest.mark.parametrize("name", list(SMALL))
def test_primitive_alone_is_the_restatement_bit_for_bit(name, pool):
    index, pair = small_world(name)
    pd = lambda a, b: pair[a, b]  # noqa: E731
    launches, n_calls = index.stat("diverse_launches"), 0
    for with_counts in (True, False):  # (False: d_counts_in is NULL, presence by the pad id, pads in the middle)
        ids, dists, counts, statuses = DC.synthetic_lists(pool, with_counts, seed=100 * pool + with_counts)
        stats = np.random.default_rng(pool).integers(2 ** 31, 2 ** 32, (DC.NQ, 4)).astype(np.int64)
        stats[:, 3] = statuses  # (query 4 failed: count 0, padded rows, its record kept)
        for n_out in DC.n_outs(pool):
            k = DC.n_queries(pool, n_out)
            cut = lambda a: None if a is None else a[:k]  # noqa: E731
            for lam in DC.LAMBDAS:
                what = "%s pool=%d counts=%s n_out=%d lambda=%g" % (name, pool, with_counts, n_out, lam)
                got, log = select_on_device(index, cut(ids), cut(dists), cut(counts), cut(stats), n_out, lam)
                n_calls += 1
                assert dict(log) == {kernel_of(index): 1}, (what, dict(log))
                want = H.mmr_select(cut(ids), cut(dists), cut(counts), cut(statuses), pd, lam, n_out, n_points=N_SMALL)
                DC.assert_diverse_equal(got, want, what)
                want_stats = cut(stats).copy()
                want_stats[:, :3] &= 0xFFFFFFFF
                got[4][:, :3] &= 0xFFFFFFFF
                assert np.array_equal(got[4], want_stats), what
        # without stats, gaps and the optional count output: the same rows (query 4 is an ordinary one here)
        n_out = DC.n_outs(pool)[-2] if pool > 1 else 1
        got, log = select_on_device(index, ids, dists, counts, None, n_out, 0.5, want_gaps=False, want_counts=False)
        n_calls += 1
        want = H.mmr_select(ids, dists, counts, None, pd, 0.5, n_out, n_points=N_SMALL)
        DC.assert_diverse_equal((got[0], got[1], want[2], want[3]), want, "bare, %s pool=%d" % (name, pool))
        assert got[2] is None and got[3] is None and got[4] is None and dict(log) == {kernel_of(index): 1}
    assert index.stat("diverse_launches") == launches + n_calls and index.stat("diverse_calls") == 0


@pytest.mark.parametrize("name", list(SMALL))
def test_an_id_beyond_the_index_fails_its_query_alone(name):
    index, pair = small_world(name)
    pd = lambda a, b: pair[a, b]  # noqa: E731
    pool, n_out = 65, 10
    for with_counts in (True, False):
        ids, dists, counts, statuses = DC.synthetic_lists(pool, with_counts, seed=7)
        ids[1, 64], ids[3, 2], ids[7, 40] = N_SMALL, 0x80000000, N_SMALL + 5
        if with_counts:
            ids[6, 0] = MAX  # (with counts the pad id is an id like any other: beyond the index)
            counts[6], counts[7] = 3, 40  # (query 7's bad id lies beyond its count: not present)
        else:
            ids[7, 40] = MAX
        stats = np.zeros((DC.NQ, 4), dtype=np.int64)
        stats[:, 3] = statuses
        got, log = select_on_device(index, ids, dists, counts, stats, n_out, 0.5)
        want = H.mmr_select(ids, dists, counts, statuses, pd, 0.5, n_out, n_points=N_SMALL)
        bad = [1, 3, 6] if with_counts else [1, 3]
        assert np.flatnonzero(want[4] == _lib.ERR_ARG).tolist() == bad
        DC.assert_diverse_equal(got, want, "%s counts=%s" % (name, with_counts))
        assert np.array_equal(got[4][:, 3], want[4])
        for q in bad:
            assert got[3][q] == 0 and (got[0][q] == MAX).all() and np.isposinf(got[1][q]).all() and np.isposinf(got[2][q]).all()
        assert got[3][7] == n_out and got[3][2] == n_out
        assert dict(log) == {kernel_of(index): 1}


# ---- 2. the entry point against the oracle's search and distance -------------------------------------------------------
N_OUT, POOL, EF, LAM, NQ = 10, 64, 128, 0.5, 64
SEARCH = {"f32-16": (H.VEC_F32, 3000, 16), "quant8-16": (H.VEC_QUANT8, 3000, 16), "f32-100": (H.VEC_F32, 2000, 100)}


@functools.lru_cache(maxsize=None)
def search_world(name):
    """clustered rows (tests/diverse_cases.py), 64 queries, the oracle holding the product's graph, and what the oracle
    alone says: its candidates and their selection.  Built once, shared, left unchanged (a test that deletes ids puts
    them back)."""
    kind, n, d = SEARCH[name]
    rows, lonely = DC.clustered_rows(n, d, 71)
    Q = DC.clustered_queries(rows, lonely, NQ, 72)
    lv = O.draw_levels(n, M, 7)
    index = H.HNSW.new(M, 32, d, kind).insert_bulk(rows, 4, False, levels=lv)
    index.set_labels((np.arange(n) % 7).astype(np.uint32))
    orc = oracle_from_product(index, rows, lv)
    cand = orc.search_batch(Q, POOL, EF)
    want = H.mmr_select(cand[0], cand[1], cand[2], None, orc.distance, LAM, N_OUT)
    for a in (rows, Q) + tuple(want):
        a.setflags(write=False)
    return index, orc, Q, cand, want


@pytest.mark.parametrize("name", list(SEARCH))
def test_search_is_the_selection_of_the_oracles_candidates(name):
    index, orc, Q, cand, want = search_world(name)
    # the coverage the case is there for, met by the oracle alone
    differ = sum(set(want[0][q].tolist()) != set(np.asarray(cand[0])[q, :N_OUT].tolist()) for q in range(NQ))
    assert differ >= 16 and NQ - differ >= 4, (differ, NQ - differ)
    got = index.search_batch_diverse(Q, N_OUT, POOL, EF, LAM)
    DC.assert_diverse_equal(got, want, name)
    assert np.array_equal(got[4][:, :3], np.asarray(cand[3]).astype(np.int64)[:, :3]) and (got[4][:, 3] == 0).all()
    assert (got[3] == N_OUT).all() and np.isposinf(got[2][:, 0]).all() and (got[2][:, 1:] < np.inf).all()
    # the first hit is the nearest candidate; every hit is one of the candidates
    assert np.array_equal(got[0][:, 0], np.asarray(cand[0])[:, 0])
    assert all(set(got[0][q].tolist()) <= set(np.asarray(cand[0])[q].tolist()) for q in range(NQ))


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_search_at_the_ends_of_lambda(lam):
    index, orc, Q, cand, _ = search_world("f32-16")
    got = index.search_batch_diverse(Q[:16], 5, 33, EF, lam)
    c = orc.search_batch(Q[:16], 33, EF)
    DC.assert_diverse_equal(got, H.mmr_select(c[0], c[1], c[2], None, orc.distance, lam, 5), "lambda %g" % lam)
    if lam == 1.0:  # the plain top 5
        assert np.array_equal(got[0], np.asarray(c[0])[:, :5])


# ---- 3. accounting, deletions, filters, the cosine option --------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-16", "quant8-16"])
def test_a_call_is_the_search_plus_one_selection(name):
    index, _, Q, _, want = search_world(name)
    index.search_batch_diverse(Q, N_OUT, POOL, EF, LAM)  # (the snapshot is in HBM from here on)
    with H.kernel_log() as plain:
        index.search_batch(Q, POOL, EF)
    calls, launches, uploads = index.stat("diverse_calls"), index.stat("diverse_launches"), index.stat("uploads")
    with H.kernel_log() as log:
        got = index.search_batch_diverse(Q, N_OUT, POOL, EF, LAM)
    name_k = kernel_of(index)
    assert log.get(name_k) == 1, dict(log)
    assert name_k not in plain and set(log) <= set(plain) | {name_k}, (dict(log), dict(plain))
    assert {k: v for k, v in log.items() if k != name_k} == dict(plain), "one search and its re-runs: %s" % dict(log)
    assert index.stat("diverse_calls") == calls + 1 and index.stat("diverse_launches") == launches + 1
    assert index.stat("uploads") == uploads
    DC.assert_diverse_equal(got, want, "second call")


def candidates(index, Q, pool, ef, s, mo, lo, hi):
    if s is not None and lo is not None:
        return index.search_batch_filtered_set_range(Q, pool, ef, s, mo, lo, hi)
    if s is not None:
        return index.search_batch_filtered_set(Q, pool, ef, s, mo)
    if lo is not None:
        return index.search_batch_filtered_range(Q, pool, ef, lo, hi)
    return index.search_batch(Q, pool, ef)


@pytest.mark.parametrize("name", ["f32-16", "quant8-16"])
def test_under_deletions(name):
    index, orc, Q, cand, _ = search_world(name)
    deleted = np.unique(np.asarray(cand[0])[:, ::3].reshape(-1))  # a third of what the queries would find
    index.mark_deleted(deleted)
    try:
        c = index.search_batch(Q, 64, 64)
        got = index.search_batch_diverse(Q, N_OUT, 64, 64, LAM)
        DC.assert_diverse_equal(got, H.mmr_select(c[0], c[1], c[2], None, orc.distance, LAM, N_OUT), "deleted")
        assert np.array_equal(got[4], c[3]), "stats are the candidate call's"
        assert not np.isin(got[0][got[0] != MAX], deleted).any() and (got[3] > 0).all()
        with pytest.raises(H.HnswError) as e:  # the candidate call's limit while ids are deleted
            index.search_batch_diverse(Q, N_OUT, 65, 65, LAM)
        assert e.value.code == _lib.ERR_ARG
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_diverse(Q, N_OUT, 65, 65, LAM)  # nothing deleted: the unfiltered limits again
    assert (got[3] == N_OUT).all()


@pytest.mark.parametrize("form", ["range", "set", "both"])
def test_under_a_label_range_and_a_mask_set_row(form):
    index, orc, Q, _, _ = search_world("quant8-16")
    n = index.len()
    rng = np.random.default_rng(5)
    s = index.mask_set(np.stack([rng.random(n) < 0.5, rng.random(n) < 0.3]))
    mo = (np.arange(NQ) % 3).astype(np.uint32)
    mo[mo == 2] = MAX
    lo, hi = (np.arange(NQ) % 4).astype(np.uint32), (np.arange(NQ) % 4 + 2).astype(np.uint32)
    fs, fmo, flo, fhi = {"range": (None, None, lo, hi), "set": (s, (mo % 2).astype(np.uint32), None, None),
                         "both": (s, mo, lo, hi)}[form]
    try:
        c = candidates(index, Q, 40, 64, fs, fmo, flo, fhi)
        got = index.search_batch_diverse(Q, N_OUT, 40, 64, LAM, mask_set=fs, mask_of=fmo, lo=flo, hi=fhi)
    finally:
        s.close()
    DC.assert_diverse_equal(got, H.mmr_select(c[0], c[1], c[2], None, orc.distance, LAM, N_OUT), form)
    assert np.array_equal(got[4], c[3]) and (got[3] > 0).all()
    if flo is not None:  # every hit's label lies in its query's range
        lab = np.arange(n) % 7
        for q in range(NQ):
            hit = got[0][q, :got[3][q]]
            assert ((lab[hit] >= flo[q]) & (lab[hit] <= fhi[q])).all()


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_the_cosine_option(kind):
    n, d = 2000, 16
    rows, lonely = DC.clustered_rows(n, d, 81)
    Q = DC.clustered_queries(rows, lonely, 32, 82)
    lv = O.draw_levels(n, M, 8)
    index = H.HNSW.new(M, 32, d, kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(rows, 4, False, levels=lv)
    # the oracle over rows normalised beforehand by the option's arithmetic (it quantises the unit rows itself)
    orc = oracle_from_product(index, SC.unit(rows), lv)
    c = orc.search_batch(SC.unit(Q), POOL, EF)
    got = index.search_batch_diverse(Q, N_OUT, POOL, EF, LAM)
    DC.assert_diverse_equal(got, H.mmr_select(c[0], c[1], c[2], None, orc.distance, LAM, N_OUT), "cosine")
    assert (got[3] == N_OUT).all()


# ---- 4. capture and replay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32-100", "quant8-40"])
def test_the_selection_is_captured_as_one_launch_and_replays_the_direct_calls_bytes(name):
    import torch
    index, _ = small_world(name)
    cache = {}
    lists = {"real": SC.pool_lists(31, DC.ID_SPAN), "decoy": SC.pool_lists(32, DC.ID_SPAN)}
    names = ("ids_in", "dists_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}
    shapes = {"ids": (SC.NQ, N_OUT), "dists": (SC.NQ, N_OUT), "gaps": (SC.NQ, N_OUT), "counts": (SC.NQ,), "stats": (SC.NQ, 4)}

    def enqueue(i, o, stream):
        index.diversify_device(SC.NQ, SC.POOL, N_OUT, LAM, i["ids_in"], i["dists_in"], i["counts_in"], i["stats_in"], o["ids"],
                               o["dists"], o["gaps"], o["counts"], o["stats"], stream)

    def want(which):
        if which not in cache:
            ids, dists, counts, stats = lists[which]
            pair = small_world(name)[1]
            w = H.mmr_select(ids, dists, counts, None, lambda a, b: pair[a, b], LAM, N_OUT, n_points=N_SMALL)
            cache[which] = (w[0], w[1].view(np.uint32), w[2].view(np.uint32), w[3], stats.astype(np.uint32))
        return cache[which]

    call = SC.Call(torch, "diversify", inputs, shapes, enqueue)
    call.want = want
    call.distinguishable()
    direct = {}
    for which in ("real", "decoy"):  # the direct call on the current stream
        call.load(which)
        call.poison()
        call.enqueue(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        direct[which] = call.arrays(copies=False)
        assert SC.verdict(direct[which], want(which)) is None, which
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call.load("decoy")
        s.synchronize()
    with H.kernel_log() as log:
        with torch.cuda.graph(g, stream=s):
            call.enqueue(torch.cuda.current_stream().cuda_stream)
    assert dict(log) == {kernel_of(index): 1}, "one call, one captured launch: %s" % dict(log)
    with torch.cuda.stream(s):
        for which in ("real", "decoy", "real"):
            call.load(which)
            call.poison()
            g.replay()
            s.synchronize()
            got = call.arrays(copies=False)
            assert all(np.array_equal(a, b) for a, b in zip(got, direct[which])), "replay over %s" % which
