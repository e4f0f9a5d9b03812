"""Refined search measured ("Measured").

1. The refinement launch alone: a table of 1M rows x 768-d made on the device, f32 (3.1 GB) and f16 (1.5 GB), pool 100,
   1024 queries a launch, candidate ids uniform over the table.  A window is K = 100 launches between two device events,
   rotating through 8 sets of candidate lists (2.5 GB of distinct rows at f32: beyond every cache); the cooperative
   gather and the switch-forced lane-per-row loop (HNSW_MI355X_REFINE_LANE_ROWS=1) alternate, 7 windows each after a
   warm-up of both.  Reported per dtype: ms per launch of every window, the algorithmic bytes of a launch
   (nq * pool * row_bytes + nq * full_dim * 4), the share of the 8 TB/s roofline at the median, and whether the
   cooperative gather's slowest window beats the other's fastest.  The two forms' outputs are compared bit for bit.
   (f16 rows take the lane-per-row loop either way since the run recorded in profiles/refine_probe.json, where the
   cooperative loop lost at f16: the two f16 columns of a new run are the same loop.)
2. One end-to-end pair on 250,000 clustered rows x 768-d whose coordinates fall off in scale (a 128-d prefix carries most
   of the distance): an f32 index over the first 128 coordinates plus the refinement against the full rows (f32 table,
   pool 100, ef 100), against an f32 index over all 768 coordinates (ef 100), n = 10, 4096 queries a call.  q/s: host
   clock around a call that ends in a device synchronise, the median of 5 after a warm-up.  recall@10 against
   hnsw_brute_force over the 768-d index.

usage: python scripts/refine_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

ROWS, FULL_DIM, POOL, NQ, N_OUT = 1_000_000, 768, 100, 1024, 10
K, SETS, WINDOWS = 100, 8, 7
SWITCH = "HNSW_MI355X_REFINE_LANE_ROWS"
ROOFLINE = 8e12
E2E_N, E2E_PREFIX, E2E_NQ, E2E_EF, M, EFC = 250_000, 128, 4096, 100, 16, 32


def launch_alone(torch, dtype):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn((ROWS, FULL_DIM), generator=g, device=dev, dtype=torch.float32)
    if dtype == "f16":
        table = table.half()
    Q = torch.randn((NQ, FULL_DIM), generator=g, device=dev, dtype=torch.float32)
    ids = torch.randint(0, ROWS, (SETS, NQ, POOL), generator=g, device=dev, dtype=torch.int32)
    o_ids = torch.empty((NQ, N_OUT), dtype=torch.int32, device=dev)
    o_dists = torch.empty((NQ, N_OUT), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(s):
        H.refine_device(NQ, POOL, N_OUT, FULL_DIM, dtype, table, ROWS, Q, ids[s], None, None, o_ids, o_dists, None, None, stream)

    def window(lane_rows):
        if lane_rows:
            os.environ[SWITCH] = "1"
        try:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(K):
                launch(k % SETS)
            b.record()
            torch.cuda.synchronize()
        finally:
            os.environ.pop(SWITCH, None)
        return a.elapsed_time(b) / K

    outs = {}
    for lane_rows in (False, True):  # warm-up of both, and their outputs on one set of lists
        window(lane_rows)
        if lane_rows:
            os.environ[SWITCH] = "1"
        launch(0)
        torch.cuda.synchronize()
        os.environ.pop(SWITCH, None)
        outs[lane_rows] = (o_ids.cpu().numpy().copy(), o_dists.cpu().numpy().view(np.uint32).copy())
    same = all(np.array_equal(x, y) for x, y in zip(outs[False], outs[True]))
    ms = {False: [], True: []}
    for _ in range(WINDOWS):
        for lane_rows in (False, True):
            ms[lane_rows].append(window(lane_rows))
    row_bytes = FULL_DIM * (2 if dtype == "f16" else 4)
    algo = NQ * POOL * row_bytes + NQ * FULL_DIM * 4
    share = lambda v: algo / (float(np.median(v)) * 1e-3) / ROOFLINE  # noqa: E731
    res = dict(dtype=dtype, rows=ROWS, full_dim=FULL_DIM, pool=POOL, nq=NQ, n_out=N_OUT, launches_per_window=K,
               algorithmic_bytes_per_launch=algo, cooperative_ms_per_launch=ms[False], lane_per_row_ms_per_launch=ms[True],
               cooperative_share_of_8TBps=share(ms[False]), lane_per_row_share_of_8TBps=share(ms[True]),
               cooperative_slowest_beats_lane_per_row_fastest=bool(max(ms[False]) < min(ms[True])),
               outputs_equal_bit_for_bit=bool(same))
    print(json.dumps(res), flush=True)
    del table
    torch.cuda.empty_cache()
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
    scale = (1.0 / np.sqrt(1.0 + np.arange(FULL_DIM) / 32.0)).astype(np.float32)
    centres = rng.standard_normal((512, FULL_DIM)).astype(np.float32)

    def draw(n):
        x = centres[rng.integers(0, len(centres), n)] + np.float32(0.5) * rng.standard_normal((n, FULL_DIM)).astype(np.float32)
        return np.ascontiguousarray(x * scale)

    rows, Q = draw(E2E_N), draw(E2E_NQ)
    t0 = time.time()
    full = H.HNSW.new(M, EFC, FULL_DIM, H.VEC_F32).insert_bulk_device(rows, 16, False)
    full.upload()
    t_full = time.time() - t0
    t0 = time.time()
    short = H.HNSW.new(M, EFC, E2E_PREFIX, H.VEC_F32).insert_bulk_device(np.ascontiguousarray(rows[:, :E2E_PREFIX]), 16, False)
    short.upload()
    t_short = time.time() - t0
    table = short.row_table(FULL_DIM, "f32")
    table.write(0, rows)
    exact = full.brute_force(Q[:1024], N_OUT)[0]
    recall = lambda got: float(np.mean([np.isin(e, g).mean() for g, e in zip(got[:1024], exact)]))  # noqa: E731
    got_full = full.search_batch(Q, N_OUT, E2E_EF)[0]
    got_short = short.search_batch(np.ascontiguousarray(Q[:, :E2E_PREFIX]), N_OUT, E2E_EF)[0]
    got_refined = short.search_batch_refined(table, None, Q, N_OUT, POOL, E2E_EF)[0]
    res = dict(rows=E2E_N, full_dim=FULL_DIM, prefix_dim=E2E_PREFIX, nq=E2E_NQ, n=N_OUT, pool=POOL, ef=E2E_EF,
               build_s=dict(full=t_full, prefix=t_short),
               full_index=dict(qps=host_qps(lambda: full.search_batch(Q, N_OUT, E2E_EF), E2E_NQ), recall_at_10=recall(got_full)),
               prefix_index_alone=dict(recall_at_10=recall(got_short)),
               prefix_index_refined=dict(qps=host_qps(lambda: short.search_batch_refined(table, None, Q, N_OUT, POOL, E2E_EF), E2E_NQ),
                                         recall_at_10=recall(got_refined)))
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
