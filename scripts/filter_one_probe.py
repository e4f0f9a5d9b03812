"""One-query filtered calls and the grouped exact path on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device
build, as bench.py builds it): n 10, ef 64.  Labels: 1 + id % 256 for the first 256 * 3900 ids (256 tenants of 3900 ids
each, labels 1 .. 256) and 1000 for the 1600 ids left; the dense range is [1, 256], every tenant's ids (998400).
  (a)  calls/s and p50 / p99 of the call at T in {1, 16, 64, 256} host threads, every call under its own tenant (the
       exact path) and every call under the dense range (the graph path):
         one:    hnsw_search_filtered through hnsw_bench_search_filtered_threads (this library's gathered form);
         batch1: T Python threads, each calling hnsw_search_batch_filtered_range with nq = 1 (ctypes releases the
                 interpreter lock in the call) -- what a caller had before; it runs on any commit that has labels.
  (b)  one batch of 1024 queries under G in {1, 16, 256} exact-path groups (tenants), "filter_exact_grouped" 0 and 1: the
       median of five windows after a warm-up, each window WINDOW calls ending in the call's own device synchronise.

usage: python scripts/filter_one_probe.py OUT.json [--quick] [--baseline-only]
       (GPU; --quick: T in {1, 64}, G in {16, 256}, shorter runs; --baseline-only: batch1 alone, for a commit without
       hnsw_search_filtered)"""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from scripts.filter_multi_probe import B, D, EF, N, TOPN, build  # noqa: E402

TENANTS, PER = 256, 3900
DENSE = 1000  # the label of the ids no tenant has
TS = [1, 16, 64, 256]
GS = [1, 16, 256]
WINDOW, WINDOWS = 10, 5


def labels():
    lab = np.full(N, DENSE, dtype=np.uint32)
    owned = TENANTS * PER
    lab[:owned] = 1 + (np.arange(owned) % TENANTS)
    return lab


def batch1_threads(idx, qs, lo, hi, T, seconds):
    """T Python threads, each blocked in a one-query batch call -> calls/s, p50, p99 [us]"""
    lat = [[] for _ in range(T)]
    go = threading.Event()

    def work(t):
        go.wait()
        end = time.perf_counter() + seconds
        i = t
        while time.perf_counter() < end:
            q = i % len(qs)
            t0 = time.perf_counter()
            idx.search_batch_filtered_range(qs[q:q + 1], TOPN, EF, lo[q:q + 1], hi[q:q + 1])
            lat[t].append(1e6 * (time.perf_counter() - t0))
            i += T

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    [t.start() for t in th]
    t0 = time.perf_counter()
    go.set()
    [t.join() for t in th]
    wall = time.perf_counter() - t0
    a = np.sort(np.concatenate([np.asarray(x) for x in lat]))
    return dict(calls_per_s=len(a) / wall, p50_us=float(a[len(a) // 2]), p99_us=float(a[min(len(a) - 1, int(0.99 * len(a)))]))


def one_threads(idx, qs, lo, hi, T, seconds):
    out = idx.search_filtered_threads(qs, TOPN, EF, lo, hi, T, seconds)
    calls, wall, lat = out[5], out[6], out[7]
    return dict(calls_per_s=calls / wall, p50_us=lat["p50"], p99_us=lat["p99"], paths=sorted(set(out[3].tolist())))


def grouped_batch(idx, qs, G):
    lo = (1 + np.arange(B) % G).astype(np.uint32)
    res = {}
    for opt in (0, 1):
        idx.set_option("filter_exact_grouped", opt)
        got = idx.search_batch_filtered_range(qs, TOPN, EF, lo, lo)  # warm-up
        assert (got[4] == 1).all()
        w = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(WINDOW):
                idx.search_batch_filtered_range(qs, TOPN, EF, lo, lo)
            w.append(1e3 * (time.perf_counter() - t0) / WINDOW)
        res["grouped_%d_ms" % opt] = float(np.median(w))
        res["grouped_%d_ms_all" % opt] = w
        res["ids_%d" % opt] = got[0]
    idx.set_option("filter_exact_grouped", 0)
    same = bool(np.array_equal(res.pop("ids_0"), res.pop("ids_1")))
    return dict(G=G, identical=same, **res)


def main():
    out_path = sys.argv[1]
    quick, base_only = "--quick" in sys.argv, "--baseline-only" in sys.argv
    ts = [1, 64] if quick else TS
    gs = [16, 256] if quick else GS
    seconds = 1.0 if quick else 2.0
    idx = build(H.VEC_F32)
    idx.set_labels(labels())
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D)
    tenant_lo = (1 + np.arange(B) % TENANTS).astype(np.uint32)
    dense_lo, dense_hi = np.ones(B, dtype=np.uint32), np.full(B, TENANTS, dtype=np.uint32)
    idx.search_batch_filtered_range(qs[:1], TOPN, EF, tenant_lo[:1], tenant_lo[:1])  # (the column's copy, the planner's sort)
    res = dict(index="1M x 100d f32, m 16, on-device build", n=TOPN, ef=EF, tenants=TENANTS, per_tenant=PER,
               dense_ids=int(TENANTS * PER), one_query=[], grouped_batch=[])
    for name, lo, hi in (("tenant", tenant_lo, tenant_lo), ("dense", dense_lo, dense_hi)):
        for T in ts:
            row = dict(filter=name, T=T, batch1=batch1_threads(idx, qs, lo, hi, T, seconds))
            if not base_only:
                row["one"] = one_threads(idx, qs, lo, hi, T, seconds)
            res["one_query"].append(row)
            print(json.dumps(row), flush=True)
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
    if not base_only:
        for G in gs:
            row = grouped_batch(idx, qs, G)
            res["grouped_batch"].append(row)
            print(json.dumps(row), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
