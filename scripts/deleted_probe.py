"""Deletion on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds it), per vector kind:
at deleted fractions 0, 1e-4, 0.01, 0.1, 0.5 and 0.95, batch 1024, n 10, ef 64 at the default filter_exact_max,
the call time of hnsw_search_batch (host clock around a call that ends in a device synchronise, median of 3 after a
warm-up), the path taken (deleted_* counters) and recall@10 against hnsw_brute_force over the live ids; then
hnsw_search (one query per call) at 64 threads without and with 1 % of the ids deleted.

usage: python scripts/deleted_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B, TOPN, EF = 1_000_000, 100, 16, 32, 1024, 10, 64
FRACS = [0.0, 1e-4, 0.01, 0.1, 0.5, 0.95]
REPS = 3
KEYS = ("deleted_queries_graph", "deleted_queries_exact", "deleted_overflow_exact")


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def main():
    out_path = sys.argv[1]
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, batch=B, topn=TOPN, ef=EF, reps=REPS,
                         timing="median host ms per hnsw_search_batch call of 1024 queries, ends in a device synchronise"),
           "points": [], "threads": []}
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    for kind_name in ("f32", "quant8"):
        kind = H.VEC_F32 if kind_name == "f32" else H.VEC_QUANT8
        vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
        idx = H.HNSW.new(M, EFC, D, kind)
        t0 = time.time()
        idx.insert_bulk_device(vs, 16, False)
        idx.upload()
        del vs
        print("%s index built in %.1f s" % (kind_name, time.time() - t0), flush=True)
        rng = np.random.default_rng(7)
        for frac in FRACS:
            dead = np.flatnonzero(rng.random(N) < frac) if frac > 0 else np.zeros(0, dtype=np.int64)
            idx.unmark_deleted(np.arange(N))
            idx.mark_deleted(dead)
            c0 = np.array([idx.stat(k) for k in KEYS])
            ms, (ids, _, counts, _) = timed(lambda: idx.search_batch(qs, TOPN, EF))
            paths = (np.array([idx.stat(k) for k in KEYS]) - c0) // (REPS + 1)
            gt, _ = idx.brute_force(qs, TOPN)
            hits = sum(len(set(a[:c].tolist()) & set(b.tolist())) for a, c, b in zip(ids, counts, gt))
            p = dict(kind=kind_name, deleted_fraction=frac, deleted=int(dead.size), call_ms=ms,
                     recall10=hits / (B * TOPN), mean_count=float(counts.mean()),
                     queries_per_path=dict(zip(("graph", "exact", "overflow_exact"), [int(x) for x in paths])),
                     returned_deleted=int(np.isin(ids, dead.astype(np.uint32)).sum()))
            res["points"].append(p)
            print(json.dumps(p), flush=True)
        for frac in (0.0, 0.01):
            idx.unmark_deleted(np.arange(N))
            if frac:
                idx.mark_deleted(np.flatnonzero(np.random.default_rng(8).random(N) < frac))
            _, _, calls, wall, lat = idx.search_threads(qs, TOPN, EF, 64, 3.0)
            p = dict(kind=kind_name, deleted_fraction=frac, threads=64, calls_per_s=calls / wall,
                     p50_us=lat["p50"], p99_us=lat["p99"], coalesced_max_batch=idx.stat("coalesced_max_batch"))
            res["threads"].append(p)
            print(json.dumps(p), flush=True)
        del idx
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
