"""hnsw_search_filtered on the MI355X: one query per call under a row of a resident set AND a label range, gathered with
its concurrent callers, and the grouped form of the exact path behind it.
  1. a lone call (coalesce_us = -1) equals the one-query batch call, bit for bit, under filters of every kind;
  2. concurrent calls (hnsw_bench_search_filtered_threads) each equal their lone answer, share launches, and a NaN
     query among them fails alone;
  3. the batch entry points with "filter_exact_grouped" = 1 return what they return with 0, in three launches for all
     exact-path groups instead of three per group;
  4. unfiltered hnsw_search calls from 64 threads return the oracle's ids and never join a filtered batch.
Indexes of 5000 points (the compaction has two blocks and a partial last word); path 2 needs more points than that and
comes from the 30000-point fixture of tests/test_gpu_mask_set.py with the labels of tests/test_gpu_labels.py."""
import threading

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.test_gpu_call_pattern import build
from tests.test_gpu_labels import device_call, glove_ranges, three_path_labels
from tests.test_gpu_mask_set import same, three_paths  # noqa: F401
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

N = 5000
MAX = 0xFFFFFFFF
NONE = -1


def scans(log):
    return sum(v for k, v in log.items() if k.startswith("hx_filt_scan_kernel"))


def compacts(log):
    return log.get("hx_filt_compact_kernel", 0)


def merges(log):
    return log.get("hx_filt_merge_kernel", 0)


@pytest.fixture(scope="module", params=[(H.VEC_F32, 60), (H.VEC_F32, 128), (H.VEC_QUANT8, 40)], ids=["f32-60", "f32-128", "q8-40"])
def idx5k(request):
    """5000 points, m = 16; a set of three rows: half the ids, one in fifty, none"""
    kind, d = request.param
    vs = rand_vectors(N, d, 7)
    index = H.HNSW.new(16, 32, d, kind).insert_bulk(vs, 8, False, levels=O.draw_levels(N, 16, 5))
    rng = np.random.default_rng(17)
    rows = [rng.random(N) < 0.5, rng.random(N) < 0.02, np.zeros(N, dtype=bool)]
    s = index.mask_set(rows)
    qs = rand_vectors(64, d, 8)
    index.upload()
    yield index, s, rows, qs
    s.close()


def batch_row(index, q, n, ef, lo, hi, s=None, row=None):
    """the one-query batch call the contract names -> (code, ids, dists, count, path)"""
    try:
        if s is None:
            got = index.search_batch_filtered_range(q[None, :], n, ef, [lo], [hi])
        else:
            got = index.search_batch_filtered_set_range(q[None, :], n, ef, s, [NONE if row is None else row], [lo], [hi])
    except H.HnswError as e:
        return (e.code,)
    return _lib.OK, got[0][0], got[1][0].view(np.uint32), int(got[2][0]), int(got[4][0])


def one(index, q, n, ef, lo, hi, s=None, row=None):
    try:
        ids, dists, count, path = index.search_filtered(q, n, ef, lo, hi, mask_set=s, row=row)
    except H.HnswError as e:
        return (e.code,)
    return _lib.OK, ids, dists.view(np.uint32), count, path


def assert_same_answer(a, b, what):
    assert a[0] == b[0], what
    if a[0] != _lib.OK:
        return
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4], (what, a, b)


# ---- 1. a lone call equals the batch row ----------------------------------------------------------------------------
def lone_cases(qs):
    lo, hi = glove_ranges(40)
    cases = [(qs[i], int(lo[i]), int(hi[i]), False, None) for i in range(40)]         # a range alone, the empty one among them
    cases += [(qs[40 + r], 0, MAX, True, r) for r in range(3)]                         # a row alone; row 2: A == 0
    cases += [(qs[43 + i], int(lo[i]), int(hi[i]), True, i % 3) for i in range(12)]    # a row AND a range
    cases += [(qs[55 + k], int(lo[i]), int(hi[i]), True, None) for k, i in enumerate((0, 11, 19))]  # HNSW_MASK_NONE with a set
    return cases


@pytest.mark.parametrize("deleted", [False, True], ids=["", "deleted"])
def test_a_lone_call_equals_the_batch_row(idx5k, deleted):
    index, s, rows, qs = idx5k
    index.set_labels((np.arange(N) % 7).astype(np.uint32))
    gone = np.random.default_rng(3).choice(N, 600, replace=False)
    index.set_option("coalesce_us", -1)
    index.set_option("filter_exact_max", 800)  # one label (715 ids) and the sparse row: exact; two labels and more: graph
    if deleted:
        index.mark_deleted(gone)
    try:
        seen = set()
        calls0, batches0 = index.stat("filtered_one_calls"), index.stat("filtered_one_batches")
        fam0 = {k: index.stat(k) for k in ("filtered_range_calls", "filtered_set_range_calls", "coalesced_queries")}
        made = 0
        for n in (1, 10, 64):
            for ci, (q, lo, hi, with_set, row) in enumerate(lone_cases(qs)):
                got = one(index, q, n, 64, lo, hi, s if with_set else None, row)
                made += 1
                want = batch_row(index, q, n, 64, lo, hi, s if with_set else None, row)
                assert_same_answer(got, want, (n, ci, lo, hi, with_set, row))
                seen.add(got[4])
                if deleted:
                    assert not np.isin(got[1][: got[3]], gone).any()
        assert seen == {0, 1}
        # every call was a launch of its own, counted under its own keys (the batch calls under theirs)
        assert index.stat("filtered_one_calls") - calls0 == made == index.stat("filtered_one_batches") - batches0
        assert index.stat("coalesced_queries") == fam0["coalesced_queries"]
        assert index.stat("filtered_range_calls") + index.stat("filtered_set_range_calls") - fam0["filtered_range_calls"] - \
            fam0["filtered_set_range_calls"] == made
        bad = qs[0].copy()
        bad[2] = np.nan
        for lo, hi in ((2, 2), (2, 4)):  # on the exact path and on the graph path
            got = one(index, bad, 10, 64, lo, hi)
            assert got == (_lib.ERR_NAN_INPUT,) == batch_row(index, bad, 10, 64, lo, hi)
    finally:
        if deleted:
            index.unmark_deleted(gone)
        index.set_option("coalesce_us", 30)
        index.set_option("filter_exact_max", 65536)


def test_a_lone_call_on_every_path(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    index.set_labels(three_path_labels(mask_list))
    index.set_option("coalesce_us", -1)
    index.set_option("filter_exact_max", 10)
    try:
        seen = set()
        for qi in (0, 4):
            for lo, hi in ((1, 1), (3, 3), (5, 5), (0, MAX), (9, 2)):
                got = one(index, Q[qi], 10, 64, lo, hi)
                assert_same_answer(got, batch_row(index, Q[qi], 10, 64, lo, hi), (qi, lo, hi))
                seen.add(got[4])
        assert seen == {0, 1, 2}
    finally:
        index.set_option("coalesce_us", 30)
        index.set_option("filter_exact_max", 65536)


# ---- 2. concurrent calls ----------------------------------------------------------------------------------------------
def test_concurrent_calls_on_all_three_paths(three_paths):
    """64 threads over 256 queries: dense (path 0), sparse (path 2), the six ids under 64 distinct ranges (path 1, 64
    groups) and no filter (path 0), one NaN query among them"""
    index, ridx, mask_list, Q8, _ = three_paths
    index.set_labels(three_path_labels(mask_list))
    Q = np.tile(Q8[::4], (32, 1)).copy()  # 256 queries
    lo = np.tile(np.array([1, 3, 5, 0], dtype=np.uint32), 64)
    hi = np.tile(np.array([1, 3, 5, MAX], dtype=np.uint32), 64)
    hi[2::4] = 5 + np.arange(64)  # [5, 5 + k]: the six ids each time, a group of its own each time
    Q[9, 3] = np.nan
    index.set_option("filter_exact_max", 10)
    try:
        index.set_option("coalesce_us", -1)
        lone = [batch_row(index, Q[i], 10, 64, int(lo[i]), int(hi[i])) for i in range(256)]
        assert {a[4] for a in lone if a[0] == _lib.OK} == {0, 1, 2}
        index.set_option("coalesce_us", 100000)
        calls0, batches0, co0 = index.stat("filtered_one_calls"), index.stat("filtered_one_batches"), index.stat("coalesced_queries")
        with H.kernel_log() as log:
            ids, dists, counts, paths, rcs, calls, wall, lat = index.search_filtered_threads(Q, 10, 64, lo, hi, 64, 0.0)
        assert calls == 256
        for i in range(256):
            got = (int(rcs[i]),) if rcs[i] != _lib.OK else (_lib.OK, ids[i], dists[i].view(np.uint32), int(counts[i]), int(paths[i]))
            assert_same_answer(got, lone[i], i)
        assert rcs[9] == _lib.ERR_NAN_INPUT and (np.delete(rcs, 9) == _lib.OK).all()
        n_calls, n_batches = index.stat("filtered_one_calls") - calls0, index.stat("filtered_one_batches") - batches0
        assert n_calls == 256 and 0 < n_batches < n_calls, (n_calls, n_batches)
        assert index.stat("coalesced_queries") == co0
        # per leader launch at most one compaction, one scan and one merge per pass: the planned pass and path 2's
        assert compacts(log) <= 2 * n_batches and scans(log) <= 2 * n_batches and merges(log) <= 2 * n_batches, (dict(log), n_batches)
        assert scans(log) == merges(log)
    finally:
        index.set_option("coalesce_us", 30)
        index.set_option("filter_exact_max", 65536)


def test_concurrent_calls_under_rows_and_ranges(idx5k):
    """the same with a set: a label per id, so that a range has as many ids as it is long; rows AND ranges, rows alone
    (the set's cached lists), HNSW_MASK_NONE, 48 distinct exact-path groups and the graph path"""
    index, s, rows, qs = idx5k
    index.set_labels(np.arange(N, dtype=np.uint32))
    Q = np.tile(qs, (4, 1))  # 256
    row = np.array([(i % 4) - 1 for i in range(256)])  # NONE, 0, 1, 2
    lo = np.array([37 * (i % 48) for i in range(256)], dtype=np.uint32)
    hi = (lo + 300 + (np.arange(256) % 48)).astype(np.uint32)
    lo[::5], hi[::5] = 0, MAX      # the row alone (NONE: no filter at all: 5000 ids, the graph path)
    lo[4::16], hi[4::16] = 0, 4200  # a long range without a row: 4201 ids, the graph path
    index.set_option("filter_exact_max", 3000)
    try:
        index.set_option("coalesce_us", -1)
        lone = [batch_row(index, Q[i], 10, 64, int(lo[i]), int(hi[i]), s, int(row[i])) for i in range(256)]
        assert {a[4] for a in lone} == {0, 1}
        index.set_option("coalesce_us", 100000)
        batches0 = index.stat("filtered_one_batches")
        with H.kernel_log() as log:
            ids, dists, counts, paths, rcs, calls, wall, lat = index.search_filtered_threads(Q, 10, 64, lo, hi, 64, 0.0, mask_set=s, row=row)
        assert calls == 256 and (rcs == _lib.OK).all()
        for i in range(256):
            assert_same_answer((_lib.OK, ids[i], dists[i].view(np.uint32), int(counts[i]), int(paths[i])), lone[i], i)
        n_batches = index.stat("filtered_one_batches") - batches0
        assert 0 < n_batches < 256
        assert compacts(log) <= n_batches and scans(log) <= n_batches and merges(log) <= n_batches, (dict(log), n_batches)
    finally:
        index.set_option("coalesce_us", 30)
        index.set_option("filter_exact_max", 65536)


# ---- 3. grouped against per-group through the batch entry points ----------------------------------------------------------
def exact_ranges(G, n):
    """G distinct ranges over a label per id, with A of 0, 1, n - 1, 2049 (two segments) and 4999 among them (G >= 7)"""
    base = [(10, 2058), (1, 4999), (7, 2), (5, 5), (100, 100 + n - 2), (4999, 6000), (6000, 7000)]
    fill = [(200 + 13 * k, 200 + 13 * k + 5 * (k % 9)) for k in range(G)]
    return (base + fill)[:G]


def both(index, call, want_log=None):
    """the call with the option off and on: equal; -> (result, log off, log on)"""
    index.set_option("filter_exact_grouped", 0)
    with H.kernel_log() as log0:
        a = call()
    index.set_option("filter_exact_grouped", 1)
    try:
        with H.kernel_log() as log1:
            b = call()
    finally:
        index.set_option("filter_exact_grouped", 0)
    same(a, b, "grouped against per-group")
    return a, dict(log0), dict(log1)


@pytest.mark.parametrize("G", [2, 7, 64])
@pytest.mark.parametrize("n", [1, 10, 64])
def test_grouped_equals_per_group_range(idx5k, G, n):
    index, s, rows, qs = idx5k
    index.set_labels(np.arange(N, dtype=np.uint32))
    index.set_option("filter_exact_max", 4999)
    try:
        rg = exact_ranges(G, n)
        nq = 2 * G + 2
        lo = np.array([rg[i % G][0] for i in range(nq)], dtype=np.uint32)
        hi = np.array([rg[i % G][1] for i in range(nq)], dtype=np.uint32)
        Q = np.tile(qs, (3, 1))[:nq]
        got, log0, log1 = both(index, lambda: index.search_batch_filtered_range(Q, n, 64, lo, hi))
        assert (got[4] == 1).all()
        assert (compacts(log0), scans(log0), merges(log0)) == (G, G, G), log0  # today's: per group
        assert (compacts(log1), scans(log1), merges(log1)) == (1, 1, 1), log1
        if G >= 7:
            want_counts = [min(n, a) for a in (2049, 4999, 0, 1, n - 1, 1, 0)]
            assert got[2][:7].tolist() == want_counts and got[3][:7, 0].tolist() == [2049, 4999, 0, 1, n - 1, 1, 0]
        # next to graph-path queries: one more launch, the graph kernel's
        lo[-2:], hi[-2:] = 0, MAX
        got, log0, log1 = both(index, lambda: index.search_batch_filtered_range(Q, n, 64, lo, hi))
        assert got[4].tolist() == [1] * (nq - 2) + [0, 0]
        assert (compacts(log1), scans(log1), merges(log1)) == (1, 1, 1), log1
    finally:
        index.set_option("filter_exact_max", 65536)


@pytest.mark.parametrize("G", [2, 7, 64])
def test_grouped_equals_per_group_multi_and_set(idx5k, G):
    index, s, rows, qs = idx5k
    index.set_labels(np.arange(N, dtype=np.uint32))
    rng = np.random.default_rng(100 + G)
    sizes = [0, 1, 9, 2049, 4999] + [int(x) for x in rng.integers(2, 400, size=G)]
    mask_list = []
    for a in sizes[:G] if G >= 5 else (2049, 4999):
        m = np.zeros(N, dtype=bool)
        m[rng.choice(N, a, replace=False)] = True
        mask_list.append(m)
    nq = 2 * G + 1
    mo = np.array([i % G for i in range(nq)])
    mo[-1] = NONE  # 5000 ids: the graph path
    Q = np.tile(qs, (3, 1))[:nq]
    index.set_option("filter_exact_max", 4999)
    try:
        got, log0, log1 = both(index, lambda: index.search_batch_filtered_multi(Q, 10, 64, mask_list, mo))
        assert got[4].tolist() == [1] * (nq - 1) + [0]
        assert (compacts(log0), scans(log0), merges(log0)) == (G, G, G), log0
        # (a mask without an admissible id has nothing to compact, alone among the compacted groups or not)
        assert (compacts(log1), scans(log1), merges(log1)) == (1, 1, 1), log1
        # the same masks as a resident set: equal to _multi; the first call lists the rows, the later ones compact nothing
        st = index.mask_set(mask_list)
        try:
            full_lo, full_hi = np.zeros(nq, dtype=np.uint32), np.full(nq, MAX, dtype=np.uint32)
            first = index.search_batch_filtered_set_range(Q, 10, 64, st, mo, full_lo, full_hi)
            same(first, got, "set against multi")
            c0 = index.stat("mask_set_compactions")
            got_s, log0, log1 = both(index, lambda: index.search_batch_filtered_set_range(Q, 10, 64, st, mo, full_lo, full_hi))
            same(got_s, got, "set against multi, cached lists")
            assert (compacts(log0), scans(log0), merges(log0)) == (0, G, G), log0
            assert (compacts(log1), scans(log1), merges(log1)) == (0, 1, 1), log1
            assert index.stat("mask_set_compactions") == c0
            # rows AND ranges: compacted in the scratch, every call; a row alone among them keeps its list
            lo = np.where(np.arange(nq) % 3 == 0, 0, 1000).astype(np.uint32)
            hi = np.where(np.arange(nq) % 3 == 0, MAX, 3999).astype(np.uint32)
            lo[-1], hi[-1] = 0, MAX
            got_r, log0, log1 = both(index, lambda: index.search_batch_filtered_set_range(Q, 10, 64, st, mo, lo, hi))
            n_groups = len({(int(m_), int(l), int(h_)) for m_, l, h_ in zip(mo[:-1], lo[:-1], hi[:-1])})
            assert scans(log0) == merges(log0) == n_groups and (scans(log1), merges(log1)) == (1, 1), (log0, log1)
            assert compacts(log1) <= 1 <= compacts(log0)
            for qi in range(nq - 1):
                m = mask_list[mo[qi]] & (np.arange(N) >= lo[qi]) & (np.arange(N) <= min(int(hi[qi]), N))
                assert got_r[3][qi, 0] == int(m.sum()) and got_r[4][qi] == 1, qi
        finally:
            st.close()
    finally:
        index.set_option("filter_exact_max", 65536)


def test_grouped_path_2_is_one_further_pass(three_paths):
    index, ridx, mask_list, Q, _ = three_paths
    index.set_labels(three_path_labels(mask_list))
    # dense: path 0; sparse under two names: path 2, two groups; the six ids under two names: path 1, two groups
    lo = np.tile(np.array([1, 3, 5, 0, 3, 5, 1, 0], dtype=np.uint32), 4)
    hi = np.tile(np.array([1, 3, 5, MAX, 4, 6, 1, MAX], dtype=np.uint32), 4)
    index.set_option("filter_exact_max", 10)
    try:
        got, log0, log1 = both(index, lambda: index.search_batch_filtered_range(Q, 10, 64, lo, hi))
        assert got[4].tolist() == [0, 2, 1, 0, 2, 1, 0, 0] * 4
        assert (compacts(log0), scans(log0), merges(log0)) == (4, 4, 4), log0
        assert (compacts(log1), scans(log1), merges(log1)) == (2, 2, 2), log1
        # one exact-path group and one path 2 group: the passes are what they were
        lo[4::8], hi[4::8], lo[5::8], hi[5::8] = 3, 3, 5, 5
        got, log0, log1 = both(index, lambda: index.search_batch_filtered_range(Q, 10, 64, lo, hi))
        assert (compacts(log0), scans(log0), merges(log0)) == (2, 2, 2) == (compacts(log1), scans(log1), merges(log1))
    finally:
        index.set_option("filter_exact_max", 65536)


def test_grouped_path_2_of_a_device_finish(three_paths):
    """the device form's _finish has counted nothing when a query reaches path 2: its late groups' offsets lie one behind
    the other in a lease sized on the spot, and the grouped form answers them in one pass"""
    index, ridx, mask_list, Q, _ = three_paths
    index.set_labels(three_path_labels(mask_list))
    lo = np.tile(np.array([1, 3, 5, 0, 3, 5, 1, 0], dtype=np.uint32), 4)
    hi = np.tile(np.array([1, 3, 5, MAX, 4, 6, 1, MAX], dtype=np.uint32), 4)

    def call():
        code, dev = device_call(index, Q, 10, 64, lo, hi)
        assert code is None
        return dev
    got, log0, log1 = both(index, call)
    index.set_option("filter_exact_max", -1)
    try:
        want = index.search_batch_filtered_range(Q, 10, 64, lo, hi)
    finally:
        index.set_option("filter_exact_max", 65536)
    same(got, want, "device form against the host form")
    late = {(int(l), int(h_)) for l, h_, p in zip(lo, hi, got[4]) if p == 2}
    assert len(late) >= 2, got[4]
    assert (compacts(log0), scans(log0), merges(log0)) == (len(late),) * 3, log0
    assert (compacts(log1), scans(log1), merges(log1)) == (1, 1, 1), log1


def test_a_clone_takes_filter_exact_grouped_from_its_parent():
    """hnsw_clone copies every option: a clone of a parent under "filter_exact_grouped" = 1 runs its two exact-path groups
    in three launches, a clone of a parent left at 0 in three per group, and both return the same"""
    n_pts, d, G = 600, 16, 2
    vs = rand_vectors(n_pts, d, 21)
    parent = H.HNSW.new(16, 32, d, H.VEC_F32).insert_bulk(vs, 4, False, levels=O.draw_levels(n_pts, 16, 5))
    parent.set_labels(np.arange(n_pts, dtype=np.uint32))
    parent.set_option("filter_exact_max", n_pts + 1)  # every query by the exact path
    Q = rand_vectors(6, d, 22)
    rg = [(10, 300), (250, 599)]
    lo = np.array([rg[i % G][0] for i in range(6)], dtype=np.uint32)
    hi = np.array([rg[i % G][1] for i in range(6)], dtype=np.uint32)
    got = {}
    for grouped, want in ((0, (G, G, G)), (1, (1, 1, 1))):
        parent.set_option("filter_exact_grouped", grouped)
        clone = parent.clone()
        with H.kernel_log() as log:
            got[grouped] = clone.search_batch_filtered_range(Q, 10, 64, lo, hi)
        assert (compacts(log), scans(log), merges(log)) == want, (grouped, dict(log))
        assert (got[grouped][4] == 1).all() and (got[grouped][2] == 10).all()
    same(got[0], got[1], "a clone of a grouped parent against a clone of a per-group parent")


# ---- 4. unfiltered hnsw_search next to filtered callers -----------------------------------------------------------------
def test_unfiltered_calls_keep_their_batches():
    index, orc, _, _ = build(N, 60, 16, H.VEC_F32)
    qs = H.synth_rows(0, 0x5EED0002, 0, 256, 60)
    want_ids, _, want_c, _ = orc.search_batch(qs, 10, 64)
    index.set_labels((np.arange(N) % 50).astype(np.uint32))
    index.upload()
    index.search_filtered(qs[0], 10, 64, 3, 3)  # (uploads the column)
    lo = (np.arange(256) % 50).astype(np.uint32)
    filtered = {}

    def run_filtered():
        filtered["out"] = index.search_filtered_threads(qs, 10, 64, lo, lo, 32, 0.3)
    q0, c0 = index.stat("coalesced_queries"), index.stat("filtered_one_calls")
    t = threading.Thread(target=run_filtered)
    t.start()
    ids, counts, calls, wall, lat = index.search_threads(qs, 10, 64, threads=64, seconds=0.3)
    t.join()
    assert np.array_equal(counts, want_c) and np.array_equal(ids, want_ids)
    assert index.stat("coalesced_queries") - q0 == calls  # only these calls
    f_ids, f_dists, f_counts, f_paths, f_rcs, f_calls = filtered["out"][:6]
    assert index.stat("filtered_one_calls") - c0 == f_calls and (f_rcs == _lib.OK).all()
    want = index.search_batch_filtered_range(qs, 10, 64, lo, lo)
    assert np.array_equal(f_ids, want[0]) and np.array_equal(f_counts, want[2]) and np.array_equal(f_paths, want[4])
