"""Boosted search measured ("Measured").

1. The boost launch alone beside the refinement launch, the form that existed before it: 1024 queries a launch, pool 256,
   a table of 1M rows made on the device, A = 8 attributes for the boost and full_dim = 8 for the refinement, f32 and
   f16, candidate ids uniform over the table, n_out = 10.  A window is K = 100 launches between two device events,
   rotating through 8 sets of candidate lists; the two forms alternate, 7 windows each after a warm-up of both.
   Reported per dtype: ms per launch of every window and the medians.
2. One end-to-end pair on 100,000 rows x 32-d (f32 index, m = 16): search_batch_boosted(n = 10, pool = 256) against
   search_batch(n = pool) followed by boost_lists on the host, 1024 queries a call.  q/s: host clock around a call that
   ends in a device synchronise (the host form: in the restatement's return), the median of 5 after a warm-up.  The two
   answers are compared bit for bit.

usage: python scripts/boost_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

ROWS, A, POOL, NQ, N_OUT = 1_000_000, 8, 256, 1024, 10
K, SETS, WINDOWS = 100, 8, 7
E2E_N, E2E_DIM, E2E_EF, M, EFC = 100_000, 32, 256, 16, 32


def launch_alone(torch, dtype):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn((ROWS, A), generator=g, device=dev, dtype=torch.float32)
    if dtype == "f16":
        table = table.half()
    Qfull = torch.randn((NQ, A), generator=g, device=dev, dtype=torch.float32)
    w = torch.randn((NQ, 1 + A), generator=g, device=dev, dtype=torch.float32)
    ids = torch.randint(0, ROWS, (SETS, NQ, POOL), generator=g, device=dev, dtype=torch.int32)
    dists = torch.rand((SETS, NQ, POOL), generator=g, device=dev, dtype=torch.float32)
    o_ids = torch.empty((NQ, N_OUT), dtype=torch.int32, device=dev)
    o_scores = torch.empty((NQ, N_OUT), dtype=torch.float32, device=dev)
    o_dists = torch.empty((NQ, N_OUT), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def boost(s):
        H.boost_device(NQ, POOL, N_OUT, A, dtype, table, ROWS, w, NQ, ids[s], dists[s], None, None, o_ids, o_scores, o_dists,
                       None, None, stream)

    def refine(s):
        H.refine_device(NQ, POOL, N_OUT, A, dtype, table, ROWS, Qfull, ids[s], None, None, o_ids, o_dists, None, None, stream)

    def window(launch):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(K):
            launch(k % SETS)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / K

    forms = {"boost": boost, "refine": refine}
    for launch in forms.values():  # warm-up of both
        window(launch)
    ms = {name: [] for name in forms}
    for _ in range(WINDOWS):
        for name, launch in forms.items():
            ms[name].append(window(launch))
    res = dict(dtype=dtype, rows=ROWS, n_attrs=A, pool=POOL, nq=NQ, n_out=N_OUT, launches_per_window=K,
               boost_ms_per_launch=ms["boost"], refine_ms_per_launch=ms["refine"],
               boost_median_ms=float(np.median(ms["boost"])), refine_median_ms=float(np.median(ms["refine"])))
    print(json.dumps(res), flush=True)
    return res


def host_qps(fn, nq):
    fn()  # warm-up
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return nq / float(np.median(t))


def end_to_end():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((E2E_N, E2E_DIM)).astype(np.float32)
    Q = rng.standard_normal((NQ, E2E_DIM)).astype(np.float32)
    attrs = rng.random((E2E_N, A)).astype(np.float32)
    w = rng.standard_normal(1 + A).astype(np.float32)
    w[0] = 1
    index = H.HNSW.new(M, EFC, E2E_DIM, H.VEC_F32).insert_bulk_device(rows, 16, False)
    index.upload()
    table = index.row_table(A, "f32")
    table.write(0, attrs)

    def on_device():
        return index.search_batch_boosted(table, Q, w, N_OUT, POOL, E2E_EF)

    def on_host():
        ids, dists, counts, stats = index.search_batch(Q, POOL, E2E_EF)[:4]
        return H.boost_lists(ids, dists, counts, stats[:, 3].astype(np.uint32).view(np.int32), attrs, w, N_OUT)

    a, b = on_device(), on_host()
    same = all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
               for x, y in zip(a[:4], b[:4]))
    res = dict(rows=E2E_N, dim=E2E_DIM, nq=NQ, n=N_OUT, pool=POOL, ef=E2E_EF, n_attrs=A,
               search_batch_boosted_qps=host_qps(on_device, NQ), search_batch_then_boost_lists_qps=host_qps(on_host, NQ),
               outputs_equal_bit_for_bit=bool(same))
    print(json.dumps(res), flush=True)
    return res


def main():
    import torch
    out_path = sys.argv[1]
    res = {"launch_alone": [], "timing": "device events around K launches for the launch alone; host clock around a call that "
                                         "ends in a device synchronise for q/s; medians"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for dtype in ("f32", "f16"):
        res["launch_alone"].append(launch_alone(torch, dtype))
        write()  # (kept as far as the probe got)
    res["end_to_end"] = end_to_end()
    write()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
