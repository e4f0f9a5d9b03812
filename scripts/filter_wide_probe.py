"""Wide filtered search on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device build, as bench.py builds it):
hnsw_search_batch_filtered_wide under a half mask (a row of a resident set) and under a one-tenth label range, batch
1024, at (n, ef) = (64, 256), (256, 256), (256, 512), (1024, 1024): call time (host clock around the call, which ends
in a device synchronise: query upload, the clearing of the visited set's HBM level, kernels, result copy), queries per
second, the share of queries per path, mean expansions and time per expansion.  At (64, 256) the existing
hnsw_search_batch_filtered_set_range is timed in the same session, the two calls alternating.

usage: python scripts/filter_wide_probe.py OUT.json [--quick]   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B = 1_000_000, 100, 16, 32, 1024
SHAPES = [(64, 256), (256, 256), (256, 512), (1024, 1024)]
REPS = 5


def main():
    out_path = sys.argv[1]
    n_points = 100_000 if "--quick" in sys.argv else N
    vs = H.synth_rows(0, 0x5EED0001, 0, n_points, D, 16)
    idx = H.HNSW.new(M, EFC, D, H.VEC_F32)
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    rng = np.random.default_rng(2025)
    idx.set_labels(rng.integers(0, 10, size=n_points).astype(np.uint32))
    s = idx.mask_set([rng.random(n_points) < 0.5])
    filters = {"half mask": dict(mask_set=s, mask_of=np.zeros(B, dtype=np.int64)),
               "one-tenth range": dict(lo=3, hi=3)}
    res = {"shape": dict(n=n_points, d=D, m=M, ef_cons=EFC, batch=B, reps=REPS,
                         timing="median host ms per call of 1024 queries, call ends in a device synchronise"),
           "points": []}
    for name, kw in filters.items():
        for n, ef in SHAPES:
            wide = lambda: idx.search_batch_filtered_wide(qs, n, ef, **kw)  # noqa: E731
            small = None
            if n <= 64 and ef <= 256:
                small = lambda: idx.search_batch_filtered_set_range(  # noqa: E731
                    qs, n, ef, s, kw.get("mask_of", np.full(B, -1)), kw.get("lo", 0), kw.get("hi", 0xFFFFFFFF))
            for f in (wide, small):  # warm-up
                if f:
                    out = f()
                    if f is wide:
                        got = out
            t_w, t_s = [], []
            for _ in range(REPS):  # alternating
                for f, t in ((wide, t_w), (small, t_s)):
                    if f:
                        t0 = time.perf_counter()
                        f()
                        t.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(t_w))
            p = dict(filter=name, n=n, ef=ef, wide_ms=ms, wide_qps=B / (ms * 1e-3),
                     wide_ms_all=[1e3 * x for x in t_w],
                     paths={str(k): float((got[4] == k).mean()) for k in (0, 1, 2)},
                     mean_n_exp=float(got[3][:, 1].mean()), mean_n_dist=float(got[3][:, 0].mean()),
                     call_us_per_expansion_per_query=1e3 * ms / max(1.0, float(got[3][:, 1].sum())) * B)
            if small:
                p["set_range_ms"] = 1e3 * float(np.median(t_s))
                p["set_range_ms_all"] = [1e3 * x for x in t_s]
                p["wide_over_set_range"] = ms / p["set_range_ms"]
            res["points"].append(p)
            print(json.dumps(p), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
