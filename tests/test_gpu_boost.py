"""Boosted search on the GPU (include/hnsw_mi355x.h, "boosted search"), held to the numpy restatement
(hnsw_rs_amd.boost.boost_lists; tests/test_boost_host.py holds that to a plain loop and to answers worked out by hand).
There are no tolerances: ids, score BITS, distance BITS, counts, counters and statuses.
  1. hnsw_boost_device alone over the synthetic lists of tests/boost_cases.py: every lane-stride edge of the pool, every
     load path of a row (A, both dtypes), both cuts, one weight row and one per query, counts and pads, the planted
     queries; one launch of hx_distance_kernel<1> and nothing else, guard words, no word unwritten;
  2. search_batch_boosted against the restatement over the product's own candidate call: unfiltered, under a label range,
     a mask row, both, and deletions; the cosine option; launch accounting; a short update sequence;
  3. the table's file: a bit-exact round trip through HBM for both dtypes, and a loaded table serving a search;
  4. the stream contract of the _device call (tests/stream_cases.py, tests/test_gpu_stream_contract.py::gated_call)."""
import functools

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import boost_cases as BC
from tests import stream_cases as SC
from tests.test_gpu_from_rows import guarded, unguard, up
from tests.test_gpu_stream_contract import gated_call
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
KERNEL = "hx_distance_kernel<1>"  # (the form reads nothing of the index: always the f32 instantiation)
TABLE_ROWS = 200


def bytes_up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def table_of(n_attrs, dtype):
    t = BC.make_table(TABLE_ROWS, n_attrs, dtype, 1000 * dtype + n_attrs)
    t.setflags(write=False)
    return t, bytes_up(t)


def stats_of(statuses, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 32, size=(len(statuses), 4), dtype=np.uint64).astype(np.uint32)
    s[:, 3] = np.asarray(statuses).astype(np.int64).astype(np.uint32)
    return s


# ---- 1. the primitive alone -----------------------------------------------------------------------------------------------
def boost_on_device(d_table, table_rows, n_attrs, dtype, w, ids, dists, counts, stats, n_out, extras=True):
    import torch
    nq, pool = ids.shape
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1, 1 + n_attrs)
    d_in = (up(w), up(ids), up(dists), None if counts is None else up(counts), None if stats is None else up(stats))
    sizes = {"ids": nq * n_out, "scores": nq * n_out, "dists": nq * n_out if extras else 0, "counts": nq if extras else 0,
             "stats": 0 if stats is None else nq * 4}
    out = guarded(sizes)
    torch.cuda.synchronize()
    with H.kernel_log() as log:
        H.boost_device(nq, pool, n_out, n_attrs, dtype, d_table, table_rows, d_in[0], w.shape[0], d_in[1], d_in[2], d_in[3],
                       d_in[4], out["ids"], out["scores"], out["dists"], out["counts"], out["stats"],
                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = unguard(out, sizes)
    shaped = lambda a: None if a is None else a.reshape(nq, n_out)  # noqa: E731
    return (shaped(got["ids"]), shaped(got["scores"]).view(np.float32),
            None if got["dists"] is None else shaped(got["dists"]).view(np.float32), got["counts"],
            None if got["stats"] is None else got["stats"].reshape(nq, 4)), dict(log)


@pytest.mark.parametrize("n_attrs", BC.ATTRS)
@pytest.mark.parametrize("pool", BC.POOLS)
def test_the_primitive_alone_is_the_restatement_bit_for_bit(pool, n_attrs):
    for dtype in BC.DTYPES:
        table, d_table = table_of(n_attrs, dtype)
        for with_counts, per_query in ((True, True), (False, False), (True, False), (False, True)):
            seed = 13 * pool + n_attrs + 2 * with_counts + per_query
            ids, dists, counts, statuses, w = BC.make_case(pool, table, with_counts, per_query, seed)
            stats = stats_of(statuses, seed)
            for n_out in sorted({1, pool}):
                what = "pool=%d A=%d dtype=%d counts=%s per_query=%s n_out=%d" % (pool, n_attrs, dtype, with_counts, per_query, n_out)
                want = H.boost_lists(ids, dists, counts, statuses, table, w, n_out)
                BC.check_planted(want, ids, dists, table, pool, n_out, per_query, what)  # (asked before the GPU is)
                got, log = boost_on_device(d_table, TABLE_ROWS, n_attrs, dtype, w, ids, dists, counts, stats, n_out)
                assert log == {KERNEL: 1}, (what, log)
                BC.assert_boosted_equal(got[:4], want[:4], what)
                want_stats = stats.copy()
                want_stats[:, 3] = want[4].astype(np.uint32)
                assert np.array_equal(got[4], want_stats), what  # the record passes through, but for the status
    # bare: no counts (pads mark the absent entries), no stats, no distance and no count output; a short cut
    for dtype in BC.DTYPES:
        table, d_table = table_of(n_attrs, dtype)
        ids, dists, _, _, w = BC.make_case(pool, table, False, True, 17 * pool + n_attrs)
        ids[BC.Q_FAILED] = MAX  # (without statuses the query cannot fail: it has no entry instead)
        n_out = min(10, pool)
        want = H.boost_lists(ids, dists, None, None, table, w, n_out)
        got, log = boost_on_device(d_table, TABLE_ROWS, n_attrs, dtype, w, ids, dists, None, None, n_out, extras=False)
        assert log == {KERNEL: 1} and got[2] is None and got[3] is None and got[4] is None, log
        BC.assert_boosted_equal(got[:2], want[:2], "bare: pool=%d A=%d dtype=%d" % (pool, n_attrs, dtype))


@pytest.mark.parametrize("dtype", BC.DTYPES, ids=["f32", "f16"])
def test_a_table_off_the_16_byte_grid_takes_element_loads(dtype):
    """a table whose first row starts one element behind a 16-byte boundary: whole 16-byte pieces by its width, but no
    16-byte load may touch it"""
    import torch
    n_attrs, pool = 32, 65
    table = BC.make_table(TABLE_ROWS, n_attrs, dtype, 5)
    flat = np.concatenate([np.zeros(1, dtype=table.dtype), table.reshape(-1)])
    d_flat = bytes_up(flat)
    d_table = d_flat.data_ptr() + table.dtype.itemsize
    assert d_table % 16 != 0
    ids, dists, counts, statuses, w = BC.make_case(pool, table, True, True, 9)
    stats = stats_of(statuses, 9)
    want = H.boost_lists(ids, dists, counts, statuses, table, w, pool)
    got, log = boost_on_device(d_table, TABLE_ROWS, n_attrs, dtype, w, ids, dists, counts, stats, pool)
    assert log == {KERNEL: 1}
    BC.assert_boosted_equal(got[:4], want[:4], "off the grid, dtype=%d" % dtype)
    torch.cuda.synchronize()
    del d_flat


# ---- 2. the search ----------------------------------------------------------------------------------------------------------
N_INDEX, DIM, A, NQ, N_OUT, EF = 2000, 16, 5, 16, 10, 48


def attributes(n, seed):
    """age in days, popularity, in stock, a demotion flag, a price: what a serving layer ranks by"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 400, n), rng.random(n) * 8, rng.integers(0, 2, n), rng.random(n) < 0.05,
                     rng.random(n) * 100], axis=1).astype(np.float32)


WEIGHTS = np.array([1.0, 0.004, -0.25, -0.5, 3.0, 0.01], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def world(kind):
    """a 2 000 x 16d index of either vector kind, m = 8, with labels, and its attributes in an f16 table (quant8) or an f32
    one (f32).  Built once, left unchanged (a test that deletes ids puts them back)"""
    vs = rand_vectors(N_INDEX, DIM, 31 + kind)
    index = H.HNSW.new(8, 32, DIM, kind).insert_bulk(vs, 4, False, levels=O.draw_levels(N_INDEX, 8, 31))
    index.set_labels((np.arange(N_INDEX) % 7).astype(np.uint32))
    dtype = "f16" if kind == H.VEC_QUANT8 else "f32"
    attrs = attributes(N_INDEX, 5)
    tab = index.row_table(A, dtype)
    tab.write(0, attrs)
    stored = attrs.astype(np.float16) if dtype == "f16" else attrs  # what the table holds
    stored.setflags(write=False)
    return index, tab, stored


def want_boosted(cand, stored, w, n):
    """the restatement over a candidate call's answer -> (ids, scores, dists, counts, stats)"""
    ids, dists, counts, stats = cand[:4]
    r = H.boost_lists(ids, dists, counts, stats[:, 3].astype(np.uint32).view(np.int32), stored, w, n)
    st = stats.copy()
    st[:, 3] = r[4] & 0xFFFFFFFF
    return r[0], r[1], r[2], r[3], st


def assert_search_equal(got, want, what):
    BC.assert_boosted_equal(got[:4], want[:4], what)
    assert np.array_equal(got[4], want[4]), what + ": the candidate call's counters do not pass through"


@pytest.mark.parametrize("kind", [H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def test_search_batch_boosted_is_the_boost_of_the_candidate_call(kind):
    index, tab, stored = world(kind)
    Q = rand_vectors(NQ, DIM, 77)
    per_query = np.tile(WEIGHTS, (NQ, 1)) * (1 + np.arange(NQ, dtype=np.float32)[:, None] / 8)
    # unfiltered: on the device; one pass of the pool and three and a bit
    for pool, w in ((64, WEIGHTS), (200, per_query)):
        efp = max(EF, pool)
        want = want_boosted(index.search_batch(Q, pool, efp), stored, w, N_OUT)
        got = index.search_batch_boosted(tab, Q, w, N_OUT, pool, EF)
        assert_search_equal(got, want, "pool %d" % pool)
        assert (got[3] == N_OUT).all()
        assert not np.array_equal(got[0], index.search_batch(Q, N_OUT, efp)[0])  # (the attributes rank otherwise)
    want = want_boosted(index.search_batch(Q, 200, 200), stored, per_query, 200)
    assert_search_equal(index.search_batch_boosted(tab, Q, per_query, 200, 200, 20), want, "n = pool = 200")
    # the second call of a shape: one boost launch, nothing uploaded
    keys = ("uploads", "boost_calls", "boost_launches", "row_table_writes")
    before = {k: index.stat(k) for k in keys}
    with H.kernel_log() as log:
        index.search_batch_boosted(tab, Q, per_query, 200, 200, 20)
    assert log[KERNEL] == 1 and sum(v for k, v in log.items() if k.startswith("hx_distance_kernel")) == 1, dict(log)
    assert {k: index.stat(k) for k in keys} == {"uploads": before["uploads"], "boost_calls": before["boost_calls"] + 1,
                                                "boost_launches": before["boost_launches"] + 1,
                                                "row_table_writes": before["row_table_writes"]}
    # under a label range, a mask row, and both: the candidates are the host form's
    pool, efp = 64, 64
    lo, hi = np.full(NQ, 2, dtype=np.uint32), np.full(NQ, 4, dtype=np.uint32)
    lo[3], hi[3] = 5, 1  # an empty range: no candidate, count 0
    rng = np.random.default_rng(5)
    s = index.mask_set(np.stack([rng.random(N_INDEX) < 0.5, rng.random(N_INDEX) < 0.3]))
    mo = (np.arange(NQ) % 3).astype(np.uint32)
    mo[mo == 2] = MAX
    want = want_boosted(index.search_batch_filtered_range(Q, pool, efp, lo, hi), stored, WEIGHTS, N_OUT)
    got = index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, pool, EF, lo=lo, hi=hi)
    assert_search_equal(got, want, "range")
    assert got[3][3] == 0 and (got[3][np.arange(NQ) != 3] == N_OUT).all()
    taken = got[0][got[0] != MAX]
    assert ((taken % 7 >= 2) & (taken % 7 <= 4)).all()
    want = want_boosted(index.search_batch_filtered_set(Q, pool, efp, s, mo), stored, per_query, N_OUT)
    assert_search_equal(index.search_batch_boosted(tab, Q, per_query, N_OUT, pool, EF, mask_set=s, mask_of=mo), want, "mask row")
    want = want_boosted(index.search_batch_filtered_set_range(Q, pool, efp, s, mo, lo, hi), stored, WEIGHTS, N_OUT)
    assert_search_equal(index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, pool, EF, mask_set=s, mask_of=mo, lo=lo, hi=hi), want,
                        "mask row and range")
    for kw in (dict(lo=lo, hi=hi), dict(mask_set=s, mask_of=mo), dict(mask_set=s, mask_of=mo, lo=lo, hi=hi)):
        with pytest.raises(H.HnswError) as e:
            index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, 65, EF, **kw)
        assert e.value.code == _lib.ERR_ARG and "pool <= 64" in str(e.value)
    # under deletions
    unfiltered = index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, pool, EF)
    dead = np.unique(unfiltered[0][:, :3])
    index.mark_deleted(dead)
    try:
        want = want_boosted(index.search_batch(Q, pool, efp), stored, WEIGHTS, N_OUT)
        got = index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, pool, EF)
        assert_search_equal(got, want, "deleted")
        assert not np.isin(got[0], dead).any() and (got[3] == N_OUT).all()
        with pytest.raises(H.HnswError) as e:
            index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, 65, EF)
        assert e.value.code == _lib.ERR_ARG and "pool <= 64" in str(e.value)
    finally:
        index.unmark_deleted(dead)
    assert_search_equal(index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, pool, EF), unfiltered, "undeleted")


def test_the_cosine_option_is_the_candidate_calls():
    n = 1200
    vs = rand_vectors(n, DIM, 91) * np.float32(3)
    index = H.HNSW.new(8, 32, DIM, H.VEC_F32)
    index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 4, False, levels=O.draw_levels(n, 8, 9))
    attrs = attributes(n, 6)
    tab = index.row_table(A, "f32")
    tab.write(0, attrs)
    Q = rand_vectors(12, DIM, 92) * np.float32(5)
    want = want_boosted(index.search_batch(Q, 32, 40), attrs, WEIGHTS, 8)  # (the search normalises Q, here as there)
    assert_search_equal(index.search_batch_boosted(tab, Q, WEIGHTS, 8, 32, 40), want, "cosine")


def test_the_boosted_answer_follows_an_insert_a_table_write_and_a_deletion():
    n, pool = 600, 32
    vs = rand_vectors(n + 1, DIM, 41)
    index = H.HNSW.new(8, 32, DIM, H.VEC_F32).insert_bulk(vs[:n], 4, False, levels=O.draw_levels(n, 8, 41))
    attrs = attributes(n + 1, 7)
    attrs[n] = (0, 8, 1, 0, 0)  # the new id: new, popular, in stock, free
    tab = index.row_table(A, "f32")
    tab.write(0, attrs[:n])
    Q = np.ascontiguousarray(vs[n:n + 1] + np.float32(0.01))  # next to the row that is inserted below

    def check(stored, what):
        want = want_boosted(index.search_batch(Q, pool, pool), stored, WEIGHTS, 5)
        got = index.search_batch_boosted(tab, Q, WEIGHTS, 5, pool, pool)
        assert_search_equal(got, want, what)
        return got

    assert n not in check(attrs[:n], "before")[0]
    assert index.insert_vec(vs[n], level=0) == n
    with pytest.raises(H.HnswError) as e:  # the table must cover the index: the new id's row is not written yet
        index.search_batch_boosted(tab, Q, WEIGHTS, 5, pool, pool)
    assert e.value.code == _lib.ERR_ARG and "600 rows, the index 601" in str(e.value)
    tab.write(n, attrs[n])
    assert check(attrs, "inserted")[0][0, 0] == n  # the nearest, and the best attributes
    attrs[n, 3] = 1  # demoted: an overwrite of the row
    attrs[n, 0] = 399
    tab.write(n, attrs[n])
    check(attrs, "row rewritten")
    index.mark_deleted(np.array([n]))
    assert n not in check(attrs, "deleted")[0]


# ---- 3. the table's file --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_table_round_trips_through_a_file_bit_for_bit_and_serves_a_search(tmp_path, dtype):
    index, _, _ = world(H.VEC_F32)
    np_dtype = np.float16 if dtype == "f16" else np.float32
    raw = attributes(N_INDEX, 8).astype(np_dtype)
    edge = [0.0, -0.0, 65504, -65504, 2.0 ** -24, -2.0 ** -14, 1 + 2.0 ** -10] if dtype == "f16" else \
        [0.0, -0.0, 3e38, -3e38, 1e-45, -1e-40, 1 + 2.0 ** -23]
    raw[3] = np.array(edge[:A], dtype=np_dtype)
    raw[4] = np.array(edge[-A:], dtype=np_dtype)
    tab = index.row_table(A, dtype)
    tab.write_raw(0, raw)
    path = tmp_path / "attrs.hxrt"
    tab.save(path)
    blob = open(path, "rb").read()
    assert len(blob) == 24 + raw.nbytes and blob[:4] == b"HXRT"
    assert blob[24:] == raw.astype(raw.dtype.newbyteorder(">")).tobytes()  # big-endian, the table's own dtype
    writes = index.stat("row_table_writes")
    back = index.load_row_table(path)
    assert (back.full_dim, back.dtype, back.rows) == (A, tab.dtype, N_INDEX) and index.stat("row_table_writes") == writes + 1
    bits = np.uint16 if dtype == "f16" else np.uint32
    assert np.array_equal(back.read(0, N_INDEX).astype(np_dtype).view(bits), raw.view(bits))  # -0, subnormals, the largest
    path2 = tmp_path / "again.hxrt"
    back.save(path2)
    assert open(path2, "rb").read() == blob
    Q = rand_vectors(NQ, DIM, 78)
    a = index.search_batch_boosted(tab, Q, WEIGHTS, N_OUT, 64, EF)
    b = index.search_batch_boosted(back, Q, WEIGHTS, N_OUT, 64, EF)
    assert_search_equal(b, a, "the loaded table")
    assert_search_equal(a, want_boosted(index.search_batch(Q, 64, 64), raw, WEIGHTS, N_OUT), "the saved table")
    tab.close()
    back.close()


# ---- 4. the stream contract -----------------------------------------------------------------------------------------------
def boost_call(torch, dtype):
    """hnsw_boost_device over two sets of synthetic candidate lists and weight rows, the table resident in HBM"""
    n_attrs, pool, n_out = 31, 65, 10
    table, d_table = table_of(n_attrs, dtype)
    cases = {w: BC.make_case(pool, table, True, True, seed) for w, seed in (("real", 41), ("decoy", 42))}
    stats = {w: stats_of(cases[w][3], 43) for w in cases}
    both = lambda k: (cases["real"][k], cases["decoy"][k])  # noqa: E731
    inputs = {"ids_in": both(0), "dists_in": both(1), "counts_in": both(2), "stats_in": (stats["real"], stats["decoy"]),
              "weights": both(4)}
    shapes = {"ids": (BC.NQ, n_out), "scores": (BC.NQ, n_out), "dists": (BC.NQ, n_out), "counts": (BC.NQ,), "stats": (BC.NQ, 4)}

    def enqueue(i, o, stream):
        H.boost_device(BC.NQ, pool, n_out, n_attrs, dtype, d_table, TABLE_ROWS, i["weights"], BC.NQ, i["ids_in"], i["dists_in"],
                       i["counts_in"], i["stats_in"], o["ids"], o["scores"], o["dists"], o["counts"], o["stats"], stream)

    def want(which):
        ids, dists, counts, statuses, w = cases[which]
        r = H.boost_lists(ids, dists, counts, statuses, table, w, n_out)
        st = stats[which].copy()
        st[:, 3] = r[4].astype(np.uint32)
        return r[0], r[1].view(np.uint32), r[2].view(np.uint32), r[3], st

    call = SC.Call(torch, "boost", inputs, shapes, enqueue)
    call.want = functools.lru_cache(maxsize=None)(want)
    return call.distinguishable()


@pytest.mark.parametrize("dtype", BC.DTYPES, ids=["f32", "f16"])
def test_the_device_call_is_ordered_on_the_callers_stream_and_does_not_wait_for_it(dtype):
    import torch
    call = boost_call(torch, dtype)
    for k in range(2):  # (two streams made one after the other: tests/test_gpu_stream_contract.py says why)
        got = gated_call(torch, call, torch.cuda.Stream())
        bad = SC.verdict(got, call.want("real"), lambda: call.want("decoy"))
        assert bad is None, "boost, stream %d: %s" % (k, bad)
