"""The on-device build under the option "rows_f16" beside the plain f32 build over the SAME values.
For each shape an option handle over X and a plain handle over X16 = X.astype(float16).astype(float32) alternate, REPS
builds each, m 16, ef_construction 32, insert_bulk_device with 16 threads.  Per build: the wall time from the rows to the
first answered search (insert_bulk_device, then a search_batch of 64 queries whose results are on the host: a host clock
around work that ends synchronised), the build statistics (insert / connect kernel time, vector rows read -- turned into
algorithmic bytes and TB/s by the handle's row stride), the snapshot's bytes and uploads, and the kernels that ran.

The library is the one HNSW_MI355X_LIB names (default: this tree's), so that the same probe runs process by process on
this commit's library and on another one in one session.

--mem adds one more build per handle with a host thread sampling the device's free memory every 20 ms (its low-water mark
against the free memory before the build = the build's peak); that build's times are reported apart and not mixed in.

usage: python scripts/build16_probe.py OUT.json [--quick] [--mem] [--reps N]   (GPU)"""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd import _lib  # noqa: E402

M, EFC, NQ, K, EF = 16, 32, 64, 10, 64
SHAPES = [(1_000_000, 768), (4_000_000, 128), (1_000_000, 100)]


def one_build(rows, Q, f16, sample_mem):
    d = rows.shape[1]
    stride = 16 * -(-2 * d // 16) if f16 else (4 * d + 15) & ~15
    free0 = torch.cuda.mem_get_info()[0]
    low, stop = [free0], threading.Event()

    def sampler():
        while not stop.wait(0.02):
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])

    th = threading.Thread(target=sampler) if sample_mem else None
    if th:
        th.start()
    ix = H.HNSW.new(M, EFC, d, H.VEC_F32)
    if f16:
        ix.set_option("rows_f16", 1)
    with H.kernel_log() as log:
        t0 = time.perf_counter()
        ix.insert_bulk_device(rows, 16, False)
        t1 = time.perf_counter()
        ix.search_batch(Q, K, EF)
        t2 = time.perf_counter()
    if th:
        stop.set()
        th.join()
    st = {k: ix.stat(k) for k in ("build_insert_kernel_us", "build_connect_kernel_us", "build_rows_read", "build_batches",
                                  "build_cpu_path_points", "build_rerun_points", "snapshot_bytes", "uploads")}
    rec = dict(wall_to_first_search_s=t2 - t0, build_call_s=t1 - t0, first_search_s=t2 - t1, row_stride=stride, **st)
    rec["algorithmic_row_bytes"] = st["build_rows_read"] * stride
    rec["insert_kernel_TBps"] = rec["algorithmic_row_bytes"] / (st["build_insert_kernel_us"] * 1e-6) / 1e12
    rec["kernels"] = sorted(k for k in log if k.startswith(("hx_insert", "hx_connect", "hx_search")))
    if sample_mem:
        rec["peak_device_bytes_during_build_and_search"] = free0 - low[0]
    del ix
    return rec


def main():
    out_path = sys.argv[1]
    shapes = [(100_000, 768), (200_000, 128), (100_000, 100)] if "--quick" in sys.argv else SHAPES
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    torch.cuda.init()
    res = {"library": _lib.LIB_PATH,
           "settings": dict(m=M, ef_cons=EFC, threads=16, reps=reps, queries=NQ, n=K, ef=EF,
                            timing="host clock from the call of insert_bulk_device to the return of the first search_batch; "
                                   "the option handle and the plain handle alternate build by build"),
           "shapes": []}
    for n, d in shapes:
        X = H.synth_rows(0, 0x5EED0001, 0, n, d, 16)
        Q = H.synth_rows(0, 0x5EED0002, 0, NQ, d, 16)
        X16 = X.astype(np.float16).astype(np.float32)
        point = dict(n=n, d=d, f16=[], f32=[])
        one_build(X16[:50_000], Q, False, False), one_build(X[:50_000], Q, True, False)  # warm-up: code objects, pools
        for _ in range(reps):
            point["f16"].append(one_build(X, Q, True, False))
            point["f32"].append(one_build(X16, Q, False, False))
        if "--mem" in sys.argv:
            point["f16_sampled"] = one_build(X, Q, True, True)
            point["f32_sampled"] = one_build(X16, Q, False, True)
        for name in ("f16", "f32"):
            for key in ("wall_to_first_search_s", "build_insert_kernel_us", "build_connect_kernel_us", "insert_kernel_TBps"):
                v = [r[key] for r in point[name]]
                point["%s_%s_median_min_max" % (name, key)] = [float(np.median(v)), min(v), max(v)]
        res["shapes"].append(point)
        print(json.dumps({k: v for k, v in point.items() if k.endswith("min_max") or k in ("n", "d")}), flush=True)
        del X, X16
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
