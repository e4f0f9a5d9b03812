"""The device-pointer entry points of include/hnsw_mi355x.h held to WHERE and WHEN they run (what they compute is pinned
elsewhere):
  1. stream order: each of them enqueues on the caller's stream and returns without waiting for it -- it reads inputs
     that earlier work on that stream is still to write, and later work on that stream sees its outputs; `_finish` waits
     for the stream;
  2. capture: hnsw_merge_topk_device and hnsw_group_by_label_device are one kernel node of a graph, replayed over new
     contents of the same buffers; so is hnsw_search_batch_device within the header's conditions;
  3. concurrency: four threads on one handle through four different entry points, with the state a search brings up to
     date lazily (deleted mask, label column and its sorted copy, a mask set's words and cached lists, the scratch pool)
     first touched by all of them at once; two handles whose launches of one kernel need different LDS opt-ins.
Fixtures, expected values and the calls themselves: tests/stream_cases.py."""
import threading

import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import stream_cases as SC
from tests.util import oracle_from_product

pytestmark = pytest.mark.gpu

KINDS = {"q8": H.VEC_QUANT8, "f32": H.VEC_F32}


# ---- 1. stream order --------------------------------------------------------------------------------------------------
def gated_call(torch, call, s, finish=False, log=None):
    """The procedure of a gated case on the non-default stream s -> what the outputs held, read as the contract allows:
    warm up; prefill inputs with the decoy and outputs with poison; occupy s with the gate; on s, behind the gate, give
    the inputs their real contents; make the call; the gate must still be running when the call has returned.  Then
    either (finish=False) copy the outputs aside ON s, poison them again ON s, synchronise and return the copies, or
    (finish=True) call _finish and read the outputs on another stream with no synchronisation of the test's own."""
    with torch.cuda.stream(s):
        call.load("decoy")
        call.enqueue(s.cuda_stream)
        torch.cuda.synchronize()  # (the whole device: the warm-up is not the subject, wherever its work went)
        if call._finish is not None:
            call.finish(s.cuda_stream)
        host_s = SC.host_seconds(call, s)
        cycles, gate_s = SC.gate_cycles(torch, host_s)
        print("host time of the %s call: %.1f us (gate %.0f ms)" % (call.form, host_s * 1e6, gate_s * 1e3))
        call.load("decoy")
        call.poison()
        torch.cuda.synchronize()
        gate_done = torch.cuda.Event()
        torch.cuda._sleep(cycles)
        gate_done.record(s)
        call.load("real")
        call.enqueue(s.cuda_stream)
        still_gated = not gate_done.query()
        assert still_gated, ("the gate (%.0f ms) was over when the call returned: the call waited for the stream, or the "
                             "window for stale inputs never opened (host time of the warmed call %.1f us)"
                             % (gate_s * 1e3, host_s * 1e6))
        if not finish:
            call.take()
            s.synchronize()
            return call.arrays(copies=True)
        if log is None:
            call.finish(s.cuda_stream)
        else:
            with H.kernel_log() as seen:
                call.finish(s.cuda_stream)
            log.update(seen)
    assert torch.cuda.current_stream() != s
    return call.arrays(copies=False)  # (read on the default stream, which does not wait for s: _finish did)


ORDER_CASES = [(form, kind, "base") for form in SC.FORMS if form != "merge" for kind in KINDS]
ORDER_CASES += [("merge", "f32", "base")]  # (handle-free: no vector kind)
ORDER_CASES += [("plain", "f32", "cosine"), ("range", "f32", "cosine")]
ORDER_CASES += [(form, kind, "deleted") for form in ("plain", "set") for kind in KINDS]
FINISH_CASES = [c for c in ORDER_CASES if c[0] in SC.SEARCH_FORMS]


def case_id(c):
    return "-".join(c)


@pytest.mark.parametrize("case", ORDER_CASES, ids=case_id)
def test_the_call_is_ordered_on_the_callers_stream_and_does_not_wait_for_it(case):
    import torch
    form, kind, variant = case
    w = SC.world(KINDS[kind], variant)
    call = SC.make_call(torch, w, form)
    # Twice, on two streams made one after the other.  The runtime serves its streams from a few hardware queues (four
    # by default) and a queue runs in order: work that went to some other stream of the process is held behind the gate
    # all the same when that stream shares the caller's queue.  Observed with the filtered launch sent to the null stream:
    # some cases passed on one stream, none on both of two consecutive ones.  (An assumption about how streams are dealt
    # to queues, not a guarantee: with a single hardware queue no choice of streams would show such a launch.)
    for k in range(2):
        got = gated_call(torch, call, torch.cuda.Stream())
        bad = SC.verdict(got, call.want("real"), lambda: call.want("decoy"))
        assert bad is None, "%s, stream %d: %s" % (case_id(case), k, bad)


@pytest.mark.parametrize("case", FINISH_CASES, ids=case_id)
def test_finish_waits_for_the_callers_stream(case):
    import torch
    form, kind, variant = case
    w = SC.world(KINDS[kind], variant)
    call = SC.make_call(torch, w, form)
    got = gated_call(torch, call, torch.cuda.Stream(), finish=True)
    bad = SC.verdict(got, call.want("real"), lambda: call.want("decoy"))
    assert bad is None, "%s after _finish: %s" % (case_id(case), bad)


@pytest.mark.parametrize("form", SC.SEARCH_FORMS)
def test_finish_reruns_overflowed_queries_on_the_callers_stream(form):
    """one case per family whose _finish really launches again: walks that fill the first visited table (a hub for the
    plain form, a filter that allows fewer than efSearch ids for the others: stream_cases.rerun_world)"""
    import torch
    w = SC.rerun_world()
    call = SC.search_call(torch, w, form)
    log = {}
    got = gated_call(torch, call, torch.cuda.Stream(), finish=True, log=log)
    assert sum(log.values()) >= 1, "%s: _finish launched nothing, no query was run again" % form
    bad = SC.verdict(got, call.want("real"), lambda: call.want("decoy"))
    assert bad is None, "%s after a _finish that re-ran queries (%s): %s" % (form, dict(log), bad)


# ---- 2. capture -------------------------------------------------------------------------------------------------------
def capture_and_replay(torch, call, third, want_third, kernels):
    """capture one call on a non-default stream (one launch of a kernel whose name starts with `kernels`), replay it over
    three contents of the same input tensors"""
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call.load("decoy")
        s.synchronize()
    with H.kernel_log() as log:
        with torch.cuda.graph(g, stream=s):
            call.enqueue(torch.cuda.current_stream().cuda_stream)
    assert sum(log.values()) == 1 and all(k.startswith(kernels) for k in log), "one call, one captured launch: %s" % dict(log)
    wants = [call.want("real"), call.want("decoy"), want_third]
    with torch.cuda.stream(s):
        for k, want in enumerate(wants):
            if k < 2:
                call.load(("real", "decoy")[k])
            else:
                call.load_arrays(third)
            call.poison()
            g.replay()
            s.synchronize()
            bad = SC.verdict(call.arrays(copies=False), want)
            assert bad is None, "replay %d: %s" % (k, bad)
    return g


@pytest.mark.parametrize("with_counts,with_stats", [(True, True), (False, False)], ids=["counts-stats", "bare"])
def test_the_merge_is_captured_as_one_launch_and_replays(with_counts, with_stats):
    import torch
    call = SC.merge_call(torch, with_counts, with_stats)
    lists = SC.shard_lists(43)
    third = dict(zip(("ids_in", "dists_in", "counts_in", "stats_in"), lists))
    capture_and_replay(torch, call, third, SC.want_merge(lists, with_counts, with_stats), "hx_filt_merge_kernel")


@pytest.mark.parametrize("kind", KINDS)
def test_the_collapse_is_captured_as_one_launch_and_replays(kind):
    import torch
    w = SC.world(KINDS[kind])
    call = SC.group_call(torch, w)
    call.load("decoy")
    call.enqueue(torch.cuda.current_stream().cuda_stream)  # (the first call brings the label column to HBM: not captured)
    torch.cuda.synchronize()
    lists = SC.pool_lists(33)
    third = dict(zip(("ids_in", "dists_in", "counts_in", "stats_in"), lists))
    capture_and_replay(torch, call, third, SC.want_collapse(lists, w.labels), "hx_filt_merge_kernel")


@pytest.mark.parametrize("kind", KINDS)
def test_the_plain_search_is_captured_as_one_launch_and_replays(kind):
    """hnsw_search_batch_device within the header's conditions for capture: the snapshot current (warmed), nothing
    deleted, no cosine option, efSearch 64"""
    import torch
    w = SC.world(KINDS[kind])
    call = SC.search_call(torch, w, "plain")
    stream = torch.cuda.current_stream().cuda_stream
    call.load("decoy")
    call.enqueue(stream)
    call.finish(stream)
    third = H.synth_rows(0, 0x5EED0002, 2 * SC.NQ, SC.NQ, SC.D)
    ids, dists, counts, st = w.orc.search_batch(third, SC.TOPN, SC.EF)
    stats = np.concatenate([np.asarray(st)[:, :3], np.zeros((SC.NQ, 1))], axis=1)
    capture_and_replay(torch, call, {"Q": third}, (ids, dists.view(np.uint32), counts, stats),
                       "hx_search_kernel<%d," % KINDS[kind])


def test_the_plain_search_is_captured_at_the_edge_of_the_headers_conditions():
    """ef = 256, the largest the header promises, where the next list size would take stream-ordered scratch: f32 rows of
    128 values at m = 16 run the lean kernel with four list registers and a 32-KiB table (from ef 257 on: six registers and a
    second visited level that the launcher allocates on the caller's stream)"""
    import torch
    w = SC.capture_boundary_world()
    call = SC.search_call(torch, w, "plain", ef=SC.CAPTURE_EF)
    stream = torch.cuda.current_stream().cuda_stream
    call.load("decoy")
    call.enqueue(stream)
    call.finish(stream)
    third = H.synth_rows(0, 0x5EED0002, 2 * SC.NQ, SC.NQ, SC.CAPTURE_D)
    ids, dists, counts, st = w.orc.search_batch(third, SC.TOPN, SC.CAPTURE_EF)
    stats = np.concatenate([np.asarray(st)[:, :3], np.zeros((SC.NQ, 1))], axis=1)
    capture_and_replay(torch, call, {"Q": third}, (ids, dists.view(np.uint32), counts, stats), "hx_lean_f32_kernel<128,")


# ---- 3. concurrency across entry points ---------------------------------------------------------------------------------
ROUNDS, SLICE = 20, 8


def round_slice(r):
    lo = (r * 3) % (SC.NQ - SLICE + 1)
    return slice(lo, lo + SLICE)


def run_phase(torch, index, mask_set, w, what):
    """Four threads on `index` for ROUNDS rounds, started together and not warmed up; the expected values are those of
    the world w, which holds the same points, graph, labels, rows and deleted ids.  -> the mismatches, as text"""
    Q = w.real
    dead = w.dead.size > 0
    want_plain = w.want("plain", "real")
    want_sr = w.want("set_range", "real")
    keys = w.keys("set_range", "real")
    row1 = np.zeros(index.len(), dtype=bool)
    row1[:w.rows_b.shape[1]] = w.rows_b[1]
    want_row1 = w.walk(Q, SC.TOPN, np.tile(row1 & w.live(), (SC.NQ, 1)), exact=True)
    if dead:  # (the candidates of the grouped call are the host form's: under deletions, the exact path over the live ids)
        c = w.walk(Q, SC.POOL, np.tile(w.live(), (SC.NQ, 1)), exact=True)
    else:
        c = w.want("plain", "real", SC.POOL)
    g = H.group_by_label(c[0], c[1].view(np.float32), c[2], w.labels, SC.N_GROUPS, SC.PER_GROUP)
    want_grouped = (g[0], g[1].view(np.uint32), g[2], g[3], g[4], c[3])
    errors, barrier = [], threading.Barrier(4)

    def compare(who, r, got, want, sl):
        assert len(got) == len(want), (who, len(got), len(want))
        for k, (a, b) in enumerate(zip(got, want)):
            a = np.ascontiguousarray(a)
            a = a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a.astype(np.uint32)
            if not np.array_equal(a, np.asarray(b)[sl].astype(np.uint32).reshape(a.shape)):
                errors.append("%s: %s, round %d, output %d differs" % (what, who, r, k))

    def device_thread(form, want):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            # the thread's own buffers: all 64 queries and keys in HBM, a round's slice of them as the call's inputs
            everything = {"Q": SC.to_dev(torch, Q)}
            everything.update({k: SC.to_dev(torch, a) for k, a in (keys if form == "set_range" else {}).items()})
            i = {k: torch.empty_like(t[:SLICE]) for k, t in everything.items()}
            o = {k: torch.empty(shape, dtype=torch.int32, device=i["Q"].device) for k, shape in SC.SEARCH_OUT(SLICE, SC.TOPN).items()}
            if form == "plain":
                name = "search_batch_device"
                args = (i["Q"].data_ptr(), SLICE, SC.TOPN, SC.EF, o["ids"].data_ptr(), o["dists"].data_ptr(),
                        o["counts"].data_ptr(), o["stats"].data_ptr(), s.cuda_stream)
            else:
                name = "search_batch_filtered_set_range_device"
                args = (i["Q"], SLICE, SC.TOPN, SC.EF, mask_set, i["mask_of"], i["lo"], i["hi"], o["ids"], o["dists"], o["counts"],
                        o["stats"], s.cuda_stream)
            s.synchronize()
            barrier.wait()
            for r in range(ROUNDS):
                sl = round_slice(r)
                for k, t in i.items():
                    t.copy_(everything[k][sl], non_blocking=True)
                for t in o.values():
                    t.fill_(SC.POISON)
                getattr(index, name)(*args)
                getattr(index, name + "_finish")(*args)
                got = tuple(t.cpu().numpy().view(np.uint32) for t in o.values())
                compare(form + " device form", r, got, want, sl)

    def host_set_thread():
        barrier.wait()
        for r in range(ROUNDS):
            sl = round_slice(r)
            got = index.search_batch_filtered_set(Q[sl], SC.TOPN, SC.EF, mask_set, np.ones(SLICE, dtype=np.int64))
            if not (got[4] == 1).all():
                errors.append("%s: row 1 did not take the exact path in round %d: %s" % (what, r, got[4]))
            compare("host form under row 1", r, got[:4], want_row1, sl)

    def grouped_thread():
        barrier.wait()
        for r in range(ROUNDS):
            sl = round_slice(r)
            got = index.search_batch_grouped(Q[sl], SC.N_GROUPS, SC.PER_GROUP, SC.POOL, SC.EF)
            compare("grouped search", r, got, want_grouped, sl)

    def guarded(fn, *a):
        def run():
            try:
                fn(*a)
            except BaseException as e:  # noqa: B902 (a thread's failure is the test's)
                errors.append("%s: %s raised %r" % (what, fn.__name__, e))
                barrier.abort()
        return run

    threads = [threading.Thread(target=guarded(device_thread, "plain", want_plain)),
               threading.Thread(target=guarded(device_thread, "set_range", want_sr)),
               threading.Thread(target=guarded(host_set_thread)), threading.Thread(target=guarded(grouped_thread))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    return errors


@pytest.mark.parametrize("kind", KINDS)
def test_four_entry_points_share_one_handle_from_their_first_call_on(kind):
    """phases of four concurrent callers -- nothing deleted; 30 ids deleted; then, BETWEEN two phases and never during
    one (the contract), five more ids deleted, row 1 of the set updated, ten labels changed and one point inserted --
    every answer of every round equal to the single-threaded expectation on the state of its phase"""
    import torch
    base, deleted = SC.world(KINDS[kind]), SC.world(KINDS[kind], "deleted")
    fresh = base.index.clone()  # (a clone: nothing of it is in HBM yet, no row counted, no list cached)
    errors = run_phase(torch, fresh, fresh.mask_set(base.rows_b), base, "nothing deleted")
    assert not errors, errors[:6]

    index = base.index.clone()
    index.mark_deleted(deleted.dead)
    mset = index.mask_set(base.rows_b)
    errors = run_phase(torch, index, mset, deleted, "30 ids deleted")
    assert not errors, errors[:6]

    rng = np.random.default_rng(5)
    live = np.flatnonzero(deleted.live())
    more = rng.choice(live, 5, replace=False)
    index.mark_deleted(more)
    rows_b = base.rows_b.copy()
    on, off = np.flatnonzero(~rows_b[1])[:20], np.flatnonzero(rows_b[1])[:10]
    mset.update(1, on, True)
    mset.update(1, off, False)
    rows_b[1][on], rows_b[1][off] = True, False
    labels = np.concatenate([base.labels, np.zeros(1, dtype=np.uint32)])  # (the point to come has label 0)
    changed = rng.choice(SC.N, 10, replace=False)
    labels[changed] = (labels[changed] + 3) % SC.N_LABELS
    index.set_labels(labels[changed], ids=changed)
    v = H.synth_rows(0, 0x5EED0009, 0, 1, SC.D)
    assert index.insert_vec(v[0], level=0) == SC.N
    after = SC.World(index, np.concatenate([base.stored, v]), np.concatenate([base.levels, np.zeros(1, dtype=np.uint8)]),
                     rows_b, labels, np.concatenate([deleted.dead, more]))
    errors = run_phase(torch, index, mset, after, "after the updates between two phases")
    assert not errors, errors[:6]


# Two handles, one kernel, two LDS opt-ins.  The filtered graph kernel of f32 rows of a dimension without an instantiation
# of its own, hx_filt_graph_kernel<HNSW_VEC_F32, 0, 0, 4>, serves d = 36 and d = 768 alike.  launch_graph_r asks for
# (4 << slots_log2) + 64 R 8 + query_lds_bytes bytes; at m = 24 (rows of 48 slots) and ef' = 256, default_slots_log2 gives
# 2^14 slots, R is 4: 65536 + 2048 + 144 = 67728 bytes at d = 36 and 65536 + 2048 + 3072 = 70656 bytes at d = 768, both
# above the 48 KiB that need hipFuncSetAttribute(MaxDynamicSharedMemorySize) -- an attribute of the function, not of the
# launch, which launch_checked sets before every such launch.
LDS_M, LDS_EF, LDS_N, LDS_CALLS = 24, 256, 1500, 50
LDS_KERNEL = "hx_filt_graph_kernel<1, 0, 0, 4>"


def test_two_handles_of_different_dimension_launch_one_kernel_with_different_lds_sizes():
    worlds = []
    for d in (36, 768):
        vs = H.synth_rows(0, 0x5EED0001 + d, 0, LDS_N, d)
        lv = O.draw_levels(LDS_N, LDS_M, d)
        index = H.HNSW.new(LDS_M, 48, d, H.VEC_F32).insert_bulk(vs, 8, False, levels=lv)
        index.set_option("filter_exact_max", -1)  # every call walks the graph
        Q = H.synth_rows(0, 0x5EED0002, 0, SC.NQ, d)
        # (under a mask that allows every id, with ef >= n, the filtered search returns the plain search's ids, distance
        # bits and counters: include/hnsw_mi355x.h; the plain search's are the oracle's)
        want = oracle_from_product(index, vs, lv).search_batch(Q, SC.TOPN, LDS_EF)
        index.search_batch_filtered(Q[:1], SC.TOPN, 8, np.ones(LDS_N, dtype=bool))  # (uploads; a launch below 48 KiB)
        # the premise, pinned: the calls below launch this instantiation and no other, for both dimensions.  (Its LDS size
        # has no seam of its own: four list registers mean 128 < ef' <= 256, and at rows of 48 slots default_slots_log2
        # gives such an ef' a table of 2^14 slots, 64 KiB, whatever the dimension)
        with H.kernel_log() as log:
            index.search_batch_filtered(Q[:SLICE], SC.TOPN, LDS_EF, np.ones(LDS_N, dtype=bool))
        assert dict(log) == {LDS_KERNEL: 1}, (d, dict(log))
        assert int(index.params.mmax0) == 2 * LDS_M
        worlds.append((index, Q, want))
    errors, barrier = [], threading.Barrier(2)

    def work(index, Q, want):
        allow = np.ones(LDS_N, dtype=bool)
        for call in range(LDS_CALLS):
            sl = round_slice(call)
            try:
                barrier.wait()  # (both threads launch at the same moment, call after call)
                ids, dists, counts, stats, paths = index.search_batch_filtered(Q[sl], SC.TOPN, LDS_EF, allow)
            except H.HnswError as e:
                errors.append("d=%d call %d: error %d (%s)" % (index.dim, call, e.code, e))
                barrier.abort()
                return
            if not (np.array_equal(ids, want[0][sl]) and np.array_equal(dists.view(np.uint32), want[1][sl].view(np.uint32))
                    and np.array_equal(counts, want[2][sl]) and (paths == 0).all()
                    and np.array_equal(stats[:, :3], np.asarray(want[3])[sl, :3].astype(np.int64))):
                errors.append("d=%d call %d: the answer differs from the oracle's" % (index.dim, call))

    threads = [threading.Thread(target=work, args=w) for w in worlds]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors[:6]  # (error -5, HNSW_ERR_HIP, from a launch: the attribute of one handle's launch undid the other's)
