"""Refined search on the GPU (include/hnsw_mi355x.h, "refined search"), held to the numpy restatement
(hnsw_rs_amd.refine.refine_lists; tests/test_refine_host.py holds that to a plain loop).  All comparisons are exact: ids,
distance BITS, counts, counters and statuses.
  1. hnsw_refine_device alone over host-made lists: every load path of the kernel form and both sides of each path's
     boundary (full_dim), every pass boundary (pool), both dtypes, the planted queries and rows of tests/refine_cases.py;
     one launch of hx_distance_kernel<1> and nothing else, guard words, no word unwritten; the switch-forced lane-per-row
     loop gives the same bits;
  2. the row table: round trips, numpy's rounding, growth, holes, refused writes;
  3. search_batch_refined against the restatement over the product's own candidate call: unfiltered, under a label range,
     under deletions, under the cosine option, prefix mode, launch accounting, and recall by construction;
  4. the stream contract of the _device call (tests/stream_cases.py, tests/test_gpu_stream_contract.py::gated_call)."""
import functools
import os

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import refine_cases as RC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import guarded, unguard, up
from tests.test_gpu_stream_contract import gated_call
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
KERNEL = "hx_distance_kernel<1>"  # (the form reads nothing of the index: always the f32 instantiation)
SWITCH = "HNSW_MI355X_REFINE_LANE_ROWS"
# element loads, 16-byte loads and whole 128-byte lines, for both dtypes, and the stage loop once, K times and many times
FULL_DIMS = (1, 3, 4, 31, 32, 33, 64, 96, 100, 128, 768, 4096)
POOLS = (1, 63, 64, 65, 256, 1024)
TABLE_ROWS = 300
NQ = RC.N_PLANTED + 2


def bytes_up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=4)
def table_of(full_dim, dtype):
    t = RC.make_table(TABLE_ROWS, full_dim, dtype, 1000 * dtype + full_dim)
    t.setflags(write=False)
    return t, bytes_up(t)


def stats_of(statuses, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 32, size=(len(statuses), 4), dtype=np.uint64).astype(np.uint32)
    s[:, 3] = np.asarray(statuses).astype(np.int64).astype(np.uint32)
    return s


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def refine_on_device(d_table, table_rows, full_dim, dtype, Q, ids, counts, stats, n_out, extras=True):
    import torch
    nq, pool = ids.shape
    d_in = (up(Q), up(ids), None if counts is None else up(counts), None if stats is None else up(stats))
    sizes = {"ids": nq * n_out, "dists": nq * n_out, "counts": nq if extras else 0, "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        H.refine_device(nq, pool, n_out, full_dim, dtype, d_table, table_rows, d_in[0], d_in[1], d_in[2], d_in[3], out["ids"],
                        out["dists"], out["counts"], out["stats"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    return (got["ids"].reshape(nq, n_out), got["dists"].view(np.float32).reshape(nq, n_out), got["counts"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4)), dict(log)


def check_against_restatement(table, d_table, dtype, pool, seed, what):
    rows, full_dim = table.shape
    Q, ids, counts, statuses = RC.make_case(NQ, pool, table, True, seed)
    stats = stats_of(statuses, seed)
    want = H.refine_lists(Q, ids, counts, statuses, table, pool)
    RC.check_planted(want, pool, pool, what)  # (asked of the restatement before the GPU is)
    got, log = refine_on_device(d_table, rows, full_dim, dtype, Q, ids, counts, stats, pool)
    assert log == {KERNEL: 1}, (what, log)
    RC.assert_refined_equal(got[:3], want[:3], what)
    want_stats = stats.copy()
    want_stats[:, 3] = want[3].astype(np.uint32)
    assert np.array_equal(got[3], want_stats), what  # the record passes through, but for the status
    os.environ[SWITCH] = "1"
    try:
        forced, log = refine_on_device(d_table, rows, full_dim, dtype, Q, ids, counts, stats, pool)
    finally:
        del os.environ[SWITCH]
    assert log == {KERNEL: 1}, (what, log)
    for g, f in zip(got, forced):
        assert np.array_equal(g.view(np.uint32), f.view(np.uint32)), what + ": the lane-per-row loop gives other bits"
    # bare: no counts (pads mark the absent entries), no stats, no count output; a short cut
    Q, ids, _, _ = RC.make_case(NQ, pool, table, False, seed + 1)
    ids[RC.Q_FAILED] = MAX  # (without statuses the query cannot fail: it has no entry instead)
    n_out = min(10, pool)
    want = H.refine_lists(Q, ids, None, None, table, n_out)
    got, log = refine_on_device(d_table, rows, full_dim, dtype, Q, ids, None, None, n_out, extras=False)
    assert log == {KERNEL: 1} and got[2] is None and got[3] is None, (what, log)
    RC.assert_refined_equal(got[:2], want[:2], what + " bare")


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("full_dim", FULL_DIMS)
def test_the_primitive_alone_is_the_restatement_bit_for_bit(full_dim, dtype):
    table, d_table = table_of(full_dim, dtype)
    # every pass boundary at the widths of every load path; the long rows at the ends of the pool's range
    pools = POOLS if full_dim <= 128 else (1, 65, 1024)
    for pool in pools:
        check_against_restatement(table, d_table, dtype, pool, 7 * full_dim + pool, "full_dim=%d dtype=%d pool=%d" % (full_dim, dtype, pool))


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("full_dim", (768, 4096))
@pytest.mark.parametrize("pool", (63, 64, 256))
def test_long_rows_at_the_other_pass_boundaries(pool, full_dim, dtype):
    table, d_table = table_of(full_dim, dtype)
    check_against_restatement(table, d_table, dtype, pool, 11 * full_dim + pool, "full_dim=%d dtype=%d pool=%d" % (full_dim, dtype, pool))


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=["f32", "f16"])
def test_a_table_off_the_16_byte_grid_takes_element_loads(dtype):
    """a table whose first row starts one element behind a 16-byte boundary: whole lines by its width, but no 16-byte load
    may touch it"""
    import torch
    full_dim = 64
    table = RC.make_table(TABLE_ROWS, full_dim, dtype, 5)
    flat = np.concatenate([np.zeros(1, dtype=table.dtype), table.reshape(-1)])
    d_flat = bytes_up(flat)
    d_table = d_flat.data_ptr() + table.dtype.itemsize
    assert d_table % 16 != 0
    Q, ids, counts, statuses = RC.make_case(NQ, 65, table, True, 9)
    stats = stats_of(statuses, 9)
    want = H.refine_lists(Q, ids, counts, statuses, table, 65)
    got, log = refine_on_device(d_table, TABLE_ROWS, full_dim, dtype, Q, ids, counts, stats, 65)
    assert log == {KERNEL: 1}
    RC.assert_refined_equal(got[:3], want[:3], "off the grid, dtype=%d" % dtype)
    torch.cuda.synchronize()
    del d_flat


# ---- 2. the table ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(name):
    """funnel: an f32 index over the first 16 of 64 coordinates, the full rows in an f16 table; q8: the 8-bit kind over 40
    coordinates, the same rows at full precision in an f32 table.  Built once, left unchanged (a test that deletes ids
    puts them back)"""
    kind, dim, full_dim, dtype = {"funnel": (H.VEC_F32, 16, 64, "f16"), "q8": (H.VEC_QUANT8, 40, 40, "f32")}[name]
    n = 1500
    full = rand_vectors(n, full_dim, 31 + full_dim)
    lv = O.draw_levels(n, 16, 31)
    index = H.HNSW.new(16, 32, dim, kind).insert_bulk(full[:, :dim], 4, False, levels=lv)
    index.set_labels((np.arange(n) % 7).astype(np.uint32))
    tab = index.row_table(full_dim, dtype)
    tab.write(0, full)
    stored = full.astype(np.float16) if dtype == "f16" else full  # what the table holds
    stored.setflags(write=False)
    return index, tab, stored, full_dim, dim


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_table_round_trips_grows_and_refuses(dtype):
    index = H.HNSW.new(8, 32, 4, H.VEC_F32).insert_bulk(rand_vectors(20, 4, 1), 2, False)
    full_dim = 33
    rows = rand_vectors(400, full_dim, 2) * np.float32(30)
    rows[3, :8] = [0.0, -0.0, 65504, -65504, 2.0 ** -24, -2.0 ** -14, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11]
    held = rows.astype(np.float16).astype(np.float32) if dtype == "f16" else rows
    tab = index.row_table(full_dim, dtype)
    writes = index.stat("row_table_writes")
    tab.write(0, rows[:10])
    p0, n0 = tab.device()
    assert p0 and n0 == 10 and tab.rows == 10
    assert np.array_equal(tab.read(0, 10).view(np.uint32), held[:10].view(np.uint32))  # (f16: numpy's rounding; -0 kept)
    # growth (capacity + 1/8 does not hold 200 rows: the array moves) keeps the earlier rows; so does an append of one row
    tab.write(10, rows[10:200])
    tab.write(200, rows[200])
    assert tab.rows == 201 and tab.device()[1] == 201
    assert np.array_equal(tab.read(0, 201).view(np.uint32), held[:201].view(np.uint32))
    # an overwrite in the middle, and one that starts inside and ends beyond
    tab.write(5, rows[300:310])
    tab.write(195, rows[310:330])
    want = held[:215].copy()
    want[5:15], want[195:215] = held[300:310], held[310:330]
    assert tab.rows == 215 and np.array_equal(tab.read(0, 215).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(tab.read(7, 3).view(np.uint32), want[7:10].view(np.uint32))
    # rows already in the table's dtype
    raw = rows[330:340].astype(np.float16) if dtype == "f16" else rows[330:340]
    tab.write_raw(215, raw)
    assert np.array_equal(tab.read(215, 10).view(np.uint32), held[330:340].view(np.uint32))
    assert index.stat("row_table_writes") == writes + 6
    # a hole is refused, and a refused write changes nothing
    before, ptr_before = tab.read(0, 225), tab.device()
    with pytest.raises(H.HnswError) as e:
        tab.write(226, rows[:2])
    assert e.value.code == _lib.ERR_ARG and "hole" in str(e.value)
    bad = rows[340:350].copy()
    bad[9, 32] = np.nan
    for first in (0, 220, 225):
        with pytest.raises(H.HnswError) as e:
            tab.write(first, bad)
        assert e.value.code == _lib.ERR_NAN_INPUT
    with pytest.raises(H.HnswError) as e:
        tab.read(220, 6)
    assert e.value.code == _lib.ERR_ARG
    assert tab.rows == 225 and tab.device() == ptr_before and index.stat("row_table_writes") == writes + 6
    assert np.array_equal(tab.read(0, 225).view(np.uint32), before.view(np.uint32))
    # what the table holds is what the _device call reads
    Q = rows[350:350 + NQ].copy()
    ids = np.arange(NQ * 20, dtype=np.uint32).reshape(NQ, 20) % 225
    got, log = refine_on_device(ptr_before[0], 225, full_dim, dtype, Q, ids, None, None, 20, extras=False)
    want = H.refine_lists(Q, ids, None, None, before.astype(np.float16) if dtype == "f16" else before, 20)
    RC.assert_refined_equal(got[:2], want[:2], "the table in HBM")
    tab.close()


# ---- 3. the search ----------------------------------------------------------------------------------------------------------
N_OUT, POOL, EF = 10, 64, 48


def want_refined(cand, Qfull, stored, n):
    """the restatement over a candidate call's answer -> (ids, dists, counts, stats)"""
    ids, _, counts, stats = cand[:4]
    r = H.refine_lists(Qfull, ids, counts, stats[:, 3].astype(np.uint32).view(np.int32), stored, n)
    st = stats.copy()
    st[:, 3] = r[3] & 0xFFFFFFFF
    return r[0], r[1], r[2], st


def assert_search_equal(got, want, what):
    RC.assert_refined_equal(got[:3], want[:3], what)
    assert np.array_equal(got[3], want[3]), what + ": the candidate call's counters do not pass through"


@pytest.mark.parametrize("name", ["funnel", "q8"])
def test_search_batch_refined_is_the_refinement_of_the_candidate_call(name):
    index, tab, stored, full_dim, dim = world(name)
    Qf = rand_vectors(16, full_dim, 77)
    Q = np.ascontiguousarray(Qf[:, :dim])
    efp = max(EF, POOL)
    # unfiltered: on the device
    want = want_refined(index.search_batch(Q, POOL, efp), Qf, stored, N_OUT)
    got = index.search_batch_refined(tab, Q, Qf, N_OUT, POOL, EF)
    assert_search_equal(got, want, name)
    assert (got[2] == N_OUT).all()
    if name == "funnel":  # (16 of 64 coordinates rank otherwise than all of them)
        assert not np.array_equal(got[0], index.search_batch(Q, N_OUT, efp)[0])
    # prefix mode is passing Qfull[:, :dim]
    assert_search_equal(index.search_batch_refined(tab, None, Qf, N_OUT, POOL, EF), want, name + " prefix")
    # other queries for the index than the prefixes, n = pool, a pool that is one pass and a bit
    Q2 = rand_vectors(16, dim, 78)
    want = want_refined(index.search_batch(Q2, 100, 100), Qf, stored, 100)
    assert_search_equal(index.search_batch_refined(tab, Q2, Qf, 100, 100, 20), want, name + " n = pool = 100")
    # the second call of a shape: one refinement launch, nothing uploaded
    before = {k: index.stat(k) for k in ("uploads", "refine_calls", "refine_launches", "row_table_writes")}
    with H.kernel_log() as log:
        index.search_batch_refined(tab, Q2, Qf, 100, 100, 20)
    assert log[KERNEL] == 1 and sum(v for k, v in log.items() if k.startswith("hx_distance_kernel")) == 1, dict(log)
    after = {k: index.stat(k) for k in before}
    assert after == {"uploads": before["uploads"], "refine_calls": before["refine_calls"] + 1,
                     "refine_launches": before["refine_launches"] + 1, "row_table_writes": before["row_table_writes"]}
    # under a label range: the candidates are the host form's
    lo, hi = np.full(16, 2, dtype=np.uint32), np.full(16, 4, dtype=np.uint32)
    lo[3], hi[3] = 5, 1  # an empty range: no candidate, count 0
    cand = index.search_batch_filtered_range(Q, POOL, efp, lo, hi)
    want = want_refined(cand, Qf, stored, N_OUT)
    got = index.search_batch_refined(tab, Q, Qf, N_OUT, POOL, EF, lo=lo, hi=hi)
    assert_search_equal(got, want, name + " range")
    assert got[2][3] == 0 and (got[2][np.arange(16) != 3] == N_OUT).all()
    taken = got[0][got[0] != MAX]
    assert ((taken % 7 >= 2) & (taken % 7 <= 4)).all()
    assert_search_equal(index.search_batch_refined(tab, None, Qf, N_OUT, POOL, EF, lo=lo, hi=hi), want, name + " range, prefix")
    # under deletions
    unfiltered = index.search_batch_refined(tab, Q, Qf, N_OUT, POOL, EF)
    dead = np.unique(unfiltered[0][:, :3])
    index.mark_deleted(dead)
    try:
        want = want_refined(index.search_batch(Q, POOL, efp), Qf, stored, N_OUT)
        got = index.search_batch_refined(tab, Q, Qf, N_OUT, POOL, EF)
        assert_search_equal(got, want, name + " deleted")
        assert not np.isin(got[0], dead).any() and (got[2] == N_OUT).all()
    finally:
        index.unmark_deleted(dead)
    assert_search_equal(index.search_batch_refined(tab, Q, Qf, N_OUT, POOL, EF), unfiltered, name + " undeleted")


def test_the_cosine_option_applies_to_the_index_queries_alone():
    n, dim, full_dim = 1200, 16, 48
    full = rand_vectors(n, full_dim, 91) * np.float32(3)
    index = H.HNSW.new(16, 32, dim, H.VEC_F32)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(full[:, :dim], 4, False, levels=O.draw_levels(n, 16, 9))
    tab = index.row_table(full_dim, "f32")
    tab.write(0, full)
    Qf = rand_vectors(12, full_dim, 92) * np.float32(5)
    Q = np.ascontiguousarray(Qf[:, :dim])
    want = want_refined(index.search_batch(Q, 32, 40), Qf, full, 8)  # (the search normalises Q; Qfull is used as given)
    assert_search_equal(index.search_batch_refined(tab, Q, Qf, 8, 32, 40), want, "cosine")
    assert_search_equal(index.search_batch_refined(tab, None, Qf, 8, 32, 40), want, "cosine, prefix")


def test_refinement_never_loses_recall_against_the_head_of_its_own_pool():
    """By construction: the exact top-10 that made it into the pool are the 10 best of the pool by the full distance, so
    the refined list holds all of them, the head of the pool only those it happens to rank first"""
    n, dim, full_dim, k, pool = 4000, 16, 64, 10, 64
    rng = np.random.default_rng(17)
    centres = rng.standard_normal((40, full_dim)).astype(np.float32)
    full = (centres[rng.integers(0, 40, n)] + np.float32(0.3) * rng.standard_normal((n, full_dim)).astype(np.float32))
    Qf = (centres[rng.integers(0, 40, 16)] + np.float32(0.3) * rng.standard_normal((16, full_dim)).astype(np.float32))
    index = H.HNSW.new(16, 32, dim, H.VEC_F32).insert_bulk(full[:, :dim], 4, False, levels=O.draw_levels(n, 16, 4))
    tab = index.row_table(full_dim, "f32")
    tab.write(0, full)
    # the exact 64-d top-10 in the refinement's own arithmetic and order: the restatement over every id, a pool at a time
    best = None
    for lo in range(0, n, 1000):
        ids = np.tile(np.arange(lo, lo + 1000, dtype=np.uint32), (16, 1))
        part = H.refine_lists(Qf, ids, None, None, full, k)
        if best is None:
            best = part
            continue
        both_i, both_d = np.concatenate([best[0], part[0]], axis=1), np.concatenate([best[1], part[1]], axis=1)
        order = np.stack([np.lexsort((both_i[q], both_d[q].view(np.uint32)))[:k] for q in range(16)])
        best = (np.take_along_axis(both_i, order, 1), np.take_along_axis(both_d, order, 1))
    head = index.search_batch(np.ascontiguousarray(Qf[:, :dim]), pool, pool)[0][:, :k]
    got = index.search_batch_refined(tab, None, Qf, k, pool, pool)
    recall = lambda found: np.mean([len(set(found[q].tolist()) & set(best[0][q].tolist())) / k for q in range(16)])  # noqa: E731
    r_refined, r_head = recall(got[0]), recall(head)
    print("recall@10 against the exact 64-d top-10: refined %.4f, the head of the 16-d pool %.4f" % (r_refined, r_head))
    assert r_refined >= r_head
    for q in range(16):
        c = int(got[2][q])
        b, i = got[1][q, :c].view(np.uint32).astype(np.int64), got[0][q, :c].astype(np.int64)
        assert c == k and all(b[a] < b[a + 1] or (b[a] == b[a + 1] and i[a] < i[a + 1]) for a in range(c - 1))


# ---- 4. the stream contract -----------------------------------------------------------------------------------------------
def refine_call(torch, dtype):
    """hnsw_refine_device over two sets of synthetic candidate lists and full queries, the table resident in HBM"""
    full_dim, pool, n_out = 96, 65, 10
    table, d_table = table_of(full_dim, dtype)
    cases = {w: RC.make_case(NQ, pool, table, True, seed) for w, seed in (("real", 41), ("decoy", 42))}
    stats = {w: stats_of(cases[w][3], 43) for w in cases}
    inputs = {"Q": (cases["real"][0], cases["decoy"][0]), "ids_in": (cases["real"][1], cases["decoy"][1]),
              "counts_in": (cases["real"][2], cases["decoy"][2]), "stats_in": (stats["real"], stats["decoy"])}
    shapes = {"ids": (NQ, n_out), "dists": (NQ, n_out), "counts": (NQ,), "stats": (NQ, 4)}

    def enqueue(i, o, stream):
        H.refine_device(NQ, pool, n_out, full_dim, dtype, d_table, TABLE_ROWS, i["Q"], i["ids_in"], i["counts_in"], i["stats_in"],
                        o["ids"], o["dists"], o["counts"], o["stats"], stream)

    def want(which):
        Q, ids, counts, statuses = cases[which]
        r = H.refine_lists(Q, ids, counts, statuses, table, n_out)
        st = stats[which].copy()
        st[:, 3] = r[3].astype(np.uint32)
        return r[0], r[1].view(np.uint32), r[2], st

    call = SC.Call(torch, "refine", inputs, shapes, enqueue)
    call.want = functools.lru_cache(maxsize=None)(want)
    return call.distinguishable()


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=["f32", "f16"])
def test_the_device_call_is_ordered_on_the_callers_stream_and_does_not_wait_for_it(dtype):
    import torch
    call = refine_call(torch, dtype)
    for k in range(2):  # (two streams made one after the other: tests/test_gpu_stream_contract.py says why)
        got = gated_call(torch, call, torch.cuda.Stream())
        bad = SC.verdict(got, call.want("real"), lambda: call.want("decoy"))
        assert bad is None, "refine, stream %d: %s" % (k, bad)
