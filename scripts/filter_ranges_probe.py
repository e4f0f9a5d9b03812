"""Label-set filtered search (several label ranges per query) on the bench's index (1M x 100d f32, m 16, ef_cons 32,
on-device build, as bench.py builds it; the setup of scripts/filter_multi_probe.py): 1024 queries, n 10, ef 64.

Labels are uniform in [0, 2^20).  A list is K disjoint ranges of equal width, spread over the label space, whose union
holds a fraction s of it; a batch names G = 8 such lists (query i the list i % G, each shifted a little), for K in
{1, 2, 4, 16} and s in {0.5, 0.1, 0.01}.  Every point runs two ways:
  ranges   hnsw_search_batch_filtered_ranges -- the host call (host clock), and the graph kernel alone: device events
           around ITERS back-to-back hnsw_search_batch_filtered_ranges_device launches, the median of REPS windows after a
           warm-up, as scripts/partition_probe.py times its kernels;
  multi    what a caller pays without it: the G unions built as masks on the host (one pass over all labels per member
           and list), packed, and uploaded by hnsw_search_batch_filtered_multi -- all inside the host clock.
and records whether both gave identical ids, distances, counts, counters and paths.

--range-only: the graph-kernel time of plain hnsw_search_batch_filtered_range_device launches alone (K = 1, the three
selectivities), by the same device events: the A/B figure of a change to the filtered graph kernel.  It uses nothing newer
than the range entry points, so HNSW_MI355X_LIB may name the library of an older commit.

usage: python scripts/filter_ranges_probe.py OUT.json [--quick] [--range-only]   (GPU; --quick: K in {1, 4}, s in {0.5, 0.01})"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd import _lib  # noqa: E402
from scripts.filter_multi_probe import B, D, EF, N, TOPN, Outputs, build  # noqa: E402

KS = [1, 2, 4, 16]
SELECTIVITIES = [0.5, 0.1, 0.01]
G = 8
SPACE = 1 << 20
REPS, ITERS = 5, 10
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def lists_of(K, s):
    """G lists of K disjoint ranges each: member j of list g is [g * 37 + j * stride, ... + width - 1]"""
    stride, width = SPACE // K, max(1, int(s * SPACE) // K)
    assert width < stride or K == 1
    return [[(g * 37 + j * stride, g * 37 + j * stride + width - 1) for j in range(K)] for g in range(G)]


def window_us(torch, fn):
    """median over REPS windows of the device time of ITERS calls of fn, per call, in microseconds"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        b.synchronize()
        t.append(1e3 * a.elapsed_time(b) / ITERS)
    return float(np.median(t)), [float(x) for x in sorted(t)]


def host_ms(fn):
    fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), [float(x) for x in sorted(t)]


class DeviceBuffers:
    def __init__(self, torch, qs, lo, hi):
        dev = torch.device("cuda:0")
        u32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)  # noqa: E731
        self.q = torch.from_numpy(qs).to(dev)
        self.lo, self.hi = u32(lo), u32(hi)
        self.ids = torch.zeros((B, TOPN), dtype=torch.int32, device=dev)
        self.dists = torch.zeros((B, TOPN), dtype=torch.float32, device=dev)
        self.counts = torch.zeros(B, dtype=torch.int32, device=dev)
        self.stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)


def range_only(torch, idx, qs, out_path):
    res = {"shape": dict(n=N, d=D, batch=B, topn=TOPN, ef=EF, reps=REPS, iters=ITERS, kind="f32",
                         library=os.environ.get("HNSW_MI355X_LIB") or "this commit's",
                         timing="device events around ITERS back-to-back hnsw_search_batch_filtered_range_device launches, "
                                "median of REPS windows after a warm-up, us per launch of 1024 queries"),
           "points": []}
    for s in SELECTIVITIES:
        lists = lists_of(1, s)
        lo = np.array([lists[i % G][0][0] for i in range(B)], dtype=np.uint32)
        hi = np.array([lists[i % G][0][1] for i in range(B)], dtype=np.uint32)
        d = DeviceBuffers(torch, qs, lo, hi)
        us, windows = window_us(torch, lambda: idx.search_batch_filtered_range_device(
            d.q, B, TOPN, EF, d.lo, d.hi, d.ids, d.dists, d.counts, d.stats))
        idx.search_batch_filtered_range_device_finish(d.q, B, TOPN, EF, d.lo, d.hi, d.ids, d.dists, d.counts, d.stats)
        pt = dict(selectivity=s, range_kernel_us=us, range_kernel_us_windows=windows)
        res["points"].append(pt)
        print(json.dumps(pt), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def point(torch, idx, qs, labels, K, s):
    L, check = _lib.lib(), H.hnsw.check
    lists = lists_of(K, s)
    per_query = [lists[i % G] for i in range(B)]
    lo, hi = H.pack_ranges(per_query, B)
    mask_of = (np.arange(B) % G).astype(np.uint32)
    r_out, m_out = Outputs(B), Outputs(B)
    r_args, m_args = r_out.args(), m_out.args()

    def ranges():
        check(L.hnsw_search_batch_filtered_ranges(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, K, lo.ctypes.data_as(u32p),
                                                  hi.ctypes.data_as(u32p), *r_args))

    def multi():  # the unions as masks: built, packed and uploaded inside the clock
        words = np.stack([H.pack_allow(np.logical_or.reduce([(labels >= l) & (labels <= h) for l, h in members]))[0]
                          for members in lists])
        check(L.hnsw_search_batch_filtered_multi(idx._h, qs.ctypes.data_as(f32p), B, TOPN, EF, words.ctypes.data_as(u64p),
                                                 G, N, mask_of.ctypes.data_as(u32p), *m_args))

    ranges_ms, ranges_all = host_ms(ranges)
    multi_ms, multi_all = host_ms(multi)
    d = DeviceBuffers(torch, qs, lo, hi)
    us, windows = window_us(torch, lambda: idx.search_batch_filtered_ranges_device(
        d.q, B, TOPN, EF, K, d.lo, d.hi, d.ids, d.dists, d.counts, d.stats))
    idx.search_batch_filtered_ranges_device_finish(d.q, B, TOPN, EF, K, d.lo, d.hi, d.ids, d.dists, d.counts, d.stats)
    return dict(K=K, selectivity=s, admissible=idx.count_labels_in_ranges(lists[0]),
                paths={str(k): int((r_out.paths == k).sum()) for k in (0, 1, 2)}, identical=bool(r_out.same(m_out)),
                ranges_host_ms=ranges_ms, ranges_host_ms_all=ranges_all, multi_fresh_masks_host_ms=multi_ms,
                multi_fresh_masks_host_ms_all=multi_all, ranges_kernel_us=us, ranges_kernel_us_windows=windows)


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_ranges_probe needs a GPU")
    out_path = sys.argv[1]
    quick = "--quick" in sys.argv
    t0 = time.time()
    idx = build(H.VEC_F32)
    print("index built in %.1f s" % (time.time() - t0), flush=True)
    qs = np.ascontiguousarray(H.synth_rows(0, 0x5EED0002, 0, B, D, 16))
    labels = np.random.default_rng(2027).integers(0, SPACE, N).astype(np.uint32)
    idx.set_labels(labels)
    if "--range-only" in sys.argv:
        return range_only(torch, idx, qs, out_path)
    res = {"shape": dict(n=N, d=D, batch=B, topn=TOPN, ef=EF, reps=REPS, iters=ITERS, lists_per_batch=G, kind="f32",
                         timing="host ms for one call of 1024 queries, median of REPS after a warm-up (the multi form "
                                "builds, packs and uploads its G union masks inside the clock); kernel us: device events "
                                "around ITERS back-to-back device-form launches, median of REPS windows after a warm-up"),
           "points": []}
    for K in ([1, 4] if quick else KS):
        for s in ([0.5, 0.01] if quick else SELECTIVITIES):
            pt = point(torch, idx, qs, labels, K, s)
            res["points"].append(pt)
            print(json.dumps(pt), flush=True)
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
