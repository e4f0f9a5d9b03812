"""Radius search on the GPU (include/hnsw_mi355x.h, "radius search").  All comparisons are on ids, distance BITS, counts,
flags, rungs and stats:
  1. hnsw_radius_cut_device alone over synthetic device lists (no search) against the numpy restatement
     (hnsw_rs_amd.radius.radius_cut; tests/test_radius_host.py holds that to a naive loop), with and without a selection,
     and the kernel log: one launch of hx_filt_merge_kernel and nothing else;
  2. hnsw_search_batch_radius against radius_ladder over the CPU ORACLE's search on worlds whose expected answers cover
     every outcome of the ladder (asserted), once up to n = ef = 1024, and on a graph whose hub overflows the visited table;
  3. under deletions and with the cosine option on, against radius_ladder over the product's own search_batch;
  4. the stats."""
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from tests import radius_cases as RC
from tests.util import product_from_oracle, rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
MERGE = "hx_filt_merge_kernel"


def up(a):  # (uint32 travels as int32: the bits are what the kernel reads)
    import torch
    a = np.array(a, order="C")  # (a writable copy: the builders' arrays are read-only)
    return torch.from_numpy(a if a.dtype == np.float32 else a.view(np.int32)).to(torch.device("cuda:0"))


def cut_on_device(ids, dists, counts, stats, radius, n_out, sel=None, optional=True):
    """hnsw_radius_cut_device over uploaded lists, every output pre-filled with a sentinel -> (ids, dists, counts or
    None, flags or None, stats or None), log"""
    import torch
    dev = torch.device("cuda:0")
    nq, n_in = ids.shape
    d_in = (up(ids), up(dists), None if counts is None else up(counts), None if stats is None else up(stats.astype(np.uint32)))
    d_rad = up(np.ascontiguousarray(radius, dtype=np.float32))
    d_sel = None if sel is None else up(np.asarray(sel, dtype=np.uint32))
    o_ids = torch.full((nq, n_out), 7, dtype=torch.int32, device=dev)
    o_dists = torch.full((nq, n_out), 3.5, dtype=torch.float32, device=dev)
    o_counts = torch.full((nq,), 9, dtype=torch.int32, device=dev) if optional else None
    o_flags = torch.full((nq,), 9, dtype=torch.int32, device=dev) if optional else None
    o_stats = None if stats is None else torch.full((nq, 4), 5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        H.HNSW.radius_cut_device(nq, n_in, n_out, d_rad, d_in[0], d_in[1], d_in[2], d_in[3], o_ids, o_dists, o_counts, o_flags,
                                 o_stats, d_sel, 0 if sel is None else len(sel), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    u = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
    return (u(o_ids), o_dists.cpu().numpy(), u(o_counts), u(o_flags),
            None if o_stats is None else o_stats.cpu().numpy().astype(np.int64)), log


# ---- 1. the cut alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", RC.N_INS)
def test_cut_alone_is_the_restatement_bit_for_bit(n_in):
    for with_counts in (True, False):  # (False: d_counts_in is NULL, presence by the pad id, pads in the middle)
        ids, dists, counts, stats, radius = RC.adversarial_lists(n_in, with_counts, seed=7 * n_in + with_counts)
        for n_out in sorted({n_in, 1024}):
            what = "n_in=%d counts=%s n_out=%d" % (n_in, with_counts, n_out)
            want = H.radius_cut(ids, dists, counts, stats, radius, n_out)
            got, log = cut_on_device(ids, dists, counts, stats, radius, n_out)
            assert dict(log) == {MERGE: 1}, (what, dict(log))
            RC.assert_cut_equal(got, want, what)
            assert np.array_equal(got[4][:, :3] & 0xFFFFFFFF, stats[:, :3] & 0xFFFFFFFF) and np.array_equal(got[4][:, 3], stats[:, 3]), what
            assert got[3][0] == RC.MORE and got[2][3] == 0 and got[3][3] == 0  # the full list's flag; the failed query
            # a selection, out of order: the rows of the other queries keep the sentinel
            sel = [9, 0, 4, 2, 13]
            got, log = cut_on_device(ids, dists, counts, stats, radius, n_out, sel=sel)
            assert dict(log) == {MERGE: 1}, (what, dict(log))
            RC.assert_cut_equal(tuple(a[sel] for a in got[:4]), tuple(a[sel] for a in want[:4]), what + " selected")
            assert np.array_equal(got[4][sel, 3], stats[sel, 3])
            rest = np.setdiff1d(np.arange(RC.NQ), sel)
            assert (got[0][rest] == 7).all() and (got[1][rest] == 3.5).all() and (got[2][rest] == 9).all(), what
            assert (got[3][rest] == 9).all() and (got[4][rest] == 5).all(), what
        # without stats and without the optional outputs: the same rows (query 3 is an ordinary one here)
        want = H.radius_cut(ids, dists, counts, None, radius, n_in)
        got, log = cut_on_device(ids, dists, counts, None, radius, n_in, optional=False)
        assert dict(log) == {MERGE: 1}
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert got[2] is None and got[3] is None and got[4] is None


# ---- 2. the ladder against the oracle ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product(name, kind):
    """the product index holding the oracle's points and graph of a ladder world"""
    rows, levels, orc, _, _ = RC.world(name, kind)
    return product_from_oracle(orc, rows, levels)


def oracle_search(orc):
    return lambda q, n, ef: orc.search_batch(q, n, ef, nthreads=8)


@pytest.mark.parametrize("name,kind", [("small", H.VEC_F32), ("small", H.VEC_QUANT8), ("lean", H.VEC_F32), ("ties", H.VEC_F32)],
                         ids=["small-f32", "small-quant8", "lean-f32", "ties-f32"])
def test_ladder_is_the_oracles(name, kind):
    _, _, orc, Q, radius = RC.world(name, kind)
    index = product(name, kind)
    want = H.radius_ladder(oracle_search(orc), Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_covered(want, "%s kind %d" % (name, kind))
    index.search_batch(Q[:1], 1, 1)  # (the snapshot is in HBM from here on)
    before = {k: index.stat(k) for k in ("radius_calls", "radius_rungs", "radius_launches", "uploads")}
    with H.kernel_log() as log:
        got = index.search_batch_radius(Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_ladder_equal(got, want, "%s kind %d" % (name, kind))
    n_rungs = int(want[4].max())
    assert n_rungs == 5
    assert log.get(MERGE) == n_rungs, dict(log)
    assert sum(v for k, v in log.items() if k != MERGE) == n_rungs, dict(log)  # one search launch per rung: nothing overflows
    if name == "lean":
        assert any(k.startswith("hx_lean_f32_kernel") for k in log), dict(log)
    again = index.search_batch_radius(Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_ladder_equal(again, want, "second call")
    after = {k: index.stat(k) for k in before}
    assert after == {"radius_calls": before["radius_calls"] + 2, "radius_rungs": before["radius_rungs"] + 2 * n_rungs,
                     "radius_launches": before["radius_launches"] + 2 * n_rungs, "uploads": before["uploads"]}
    # a scalar radius is every query's; the CSR form holds the counted entries
    one = index.search_batch_radius(Q, float(radius[9]), RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_ladder_equal(one, H.radius_ladder(oracle_search(orc), Q, float(radius[9]), RC.N_FIRST, RC.MAX_N, RC.EF), "scalar")
    lims, f_ids, f_d = H.to_csr(*got[:3])
    assert lims[-1] == got[2].sum() and (f_ids != MAX).all() and np.array_equal(f_ids[lims[9]:lims[10]], got[0][9, :got[2][9]])


def test_up_to_1024_entries_every_answer_truncated():
    _, _, orc, Q, _ = RC.world("small", H.VEC_F32)
    index = product("small", H.VEC_F32)
    want = H.radius_ladder(oracle_search(orc), Q[8:12], np.inf, 256, 1024, 0)
    assert (want[3] == RC.MORE).all() and (want[2] == 1024).all() and (want[4] == 3).all()  # ef 256, 512, 1024
    got = index.search_batch_radius(Q[8:12], np.inf, 256, 1024, 0)
    RC.assert_ladder_equal(got, want, "1024")


@pytest.mark.parametrize("kind", [H.VEC_QUANT8, H.VEC_F32], ids=["quant8", "f32"])
def test_overflow_inside_the_ladder_is_rerun(kind):
    """the hub's own row as the query fills the default visited table on every rung: the rung's re-run loop answers it
    (the handled HNSW_ERR_OVERFLOW status), and the ladder goes on from the re-run's list"""
    vs, lv, orc = RC.hub_world(kind)
    index = product_from_oracle(orc, vs, lv)
    Q = np.ascontiguousarray(np.concatenate([vs[5:6], rand_vectors(24, vs.shape[1], 14)[:3]]))
    radius = orc.search_batch(Q, 16, 32)[1][:, 10].copy()  # the 11th nearest: 8 are not enough, 16 are
    want = H.radius_ladder(oracle_search(orc), Q, radius, 8, 32, 32)
    assert want[4][0] == 2 and want[3][0] == 0 and want[2][0] >= 11
    with H.kernel_log() as log:
        got = index.search_batch_radius(Q, radius, 8, 32, 32)  # (raises on a per-query error)
    RC.assert_ladder_equal(got, want, "hub, kind %d" % kind)
    assert (got[5][:, 3] == 0).all()
    n_rungs = int(want[4].max())
    assert log.get(MERGE) == n_rungs and sum(v for k, v in log.items() if k != MERGE) > n_rungs, dict(log)  # (a re-run)


# ---- 3. deletions, the cosine option --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_under_deletions(kind):
    _, _, _, Q, radius = RC.world("small", kind)
    index = product("small", kind)
    deleted = np.random.default_rng(5).choice(3000, 300, replace=False)
    index.mark_deleted(deleted)
    try:
        want = H.radius_ladder(index.search_batch, Q, radius, RC.N_FIRST, 64, RC.EF)
        got = index.search_batch_radius(Q, radius, RC.N_FIRST, 64, RC.EF)
        RC.assert_ladder_equal(got, want, "deleted, kind %d" % kind)
        assert not np.isin(got[0][got[0] != MAX], deleted).any()
        assert (got[2] == 0).any() and (got[3] == RC.MORE).any() and set(got[4].tolist()) == {1, 2, 3, 4}
        with pytest.raises(H.HnswError) as e:  # the candidate call's limit while ids are deleted
            index.search_batch_radius(Q, radius, RC.N_FIRST, 65, RC.EF)
        assert e.value.code == _lib.ERR_ARG and "max_n <= 64" in str(e.value)
    finally:
        index.unmark_deleted(deleted)
    got = index.search_batch_radius(Q, radius, RC.N_FIRST, 65, RC.EF)  # nothing deleted: the unfiltered limits again
    assert (got[4] >= 1).all()


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_with_the_cosine_option(kind):
    rows, levels, _, Q, _ = RC.world("small", kind)
    index = H.HNSW.new(8, 32, rows.shape[1], kind)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(rows, 4, False, levels=levels)
    true_d = index.search_batch(Q, RC.RANKS[-1] + 1, 512)[1]  # (near enough to the true neighbours to spread the outcomes)
    radius = np.array([true_d[i, RC.RANKS[i % 8]] for i in range(64)], dtype=np.float32)
    want = H.radius_ladder(index.search_batch, Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    assert set(want[4].tolist()) == {1, 2, 3, 4, 5} and (want[3] == RC.MORE).sum() >= 4, (want[4], want[3])  # every rung; truncation
    with H.kernel_log() as log:
        got = index.search_batch_radius(Q, radius, RC.N_FIRST, RC.MAX_N, RC.EF)
    RC.assert_ladder_equal(got, want, "cosine, kind %d" % kind)
    assert log.get("hx_normalise_rows_kernel") == 1, dict(log)  # the unit-length copy is made once, not per rung
