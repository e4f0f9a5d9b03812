"""Radius search on one MI355X at the bench's shape (1M x 100d f32, m 16, ef_cons 32, on-device build), batch 1024,
n_first 16, max_n 256, ef 0.  Query i's radius is the distance of its neighbour of rank (0, 3, 7, 8, 20, 60, 127, 168)[i % 8]
in a search with n = ef = 256, so an eighth of the batch stops at every depth of the ladder and an eighth is truncated.
Two ways to everything within the radius, a host clock around calls that end with the results on the host:
  - the ladder: hnsw_search_batch_radius (host pointers in and out);
  - one search: hnsw_search_batch at n = ef = max_n (unchanged by the radius search: the same code as before it) and
    the cut of its [B, max_n] lists on the host, by one numpy compare per list (not radius_cut, which is written to be
    checked against, not to be fast).
And the cut launch alone over [B, max_n] lists in HBM, by device events.  Each the median of REPS windows.  The two ways
are NOT the same answer where a rung's smaller ef finds other neighbours than ef = max_n does: how often they agree is
reported, not asserted; the ladder is checked against radius_ladder over search_batch before anything is timed.

usage: python scripts/radius_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B, N_FIRST, MAX_N, EF = 1_000_000, 100, 16, 32, 1024, 16, 256, 0
RANKS = (0, 3, 7, 8, 20, 60, 127, 168)
REPS, ITERS, HOST_ITERS = 5, 100, 10


def device_us(torch, fn, iters=ITERS):
    """median over REPS windows of the device time of `iters` calls of fn, per call, in microseconds"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        t.append(1e3 * a.elapsed_time(b) / iters)
    return float(np.median(t)), [float(x) for x in sorted(t)]


def host_us(torch, fn, iters=HOST_ITERS):
    """the same with a host clock around calls that end synchronised"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        t.append(1e6 * (time.perf_counter() - t0) / iters)
    return float(np.median(t)), [float(x) for x in sorted(t)]


def main():
    import torch
    out_path = sys.argv[1]
    if H.device_count() < 1:
        raise SystemExit("radius_probe needs a GPU")
    dev = torch.device("cuda:0")
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    t0 = time.time()
    index = H.HNSW.new(M, EFC, D, H.VEC_F32).insert_bulk_device(vs, 16, False)
    index.upload()
    print("built in %.1f s" % (time.time() - t0), flush=True)
    wide = index.search_batch(qs, MAX_N, MAX_N)
    radius = np.array([wide[1][i, RANKS[i % 8]] for i in range(B)], dtype=np.float32)

    def ladder():
        return index.search_batch_radius(qs, radius, N_FIRST, MAX_N, EF)

    def one_search():
        ids, dists, counts, _ = index.search_batch(qs, MAX_N, MAX_N)
        inside = (dists <= radius[:, None]) & (np.arange(MAX_N)[None, :] < counts[:, None])
        return ids, dists, inside.sum(axis=1)  # (the lists are ascending: the kept entries are a prefix)

    got = ladder()
    want = H.radius_ladder(index.search_batch, qs, radius, N_FIRST, MAX_N, EF)
    for a, b in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64),
                              np.ascontiguousarray(b).view(np.uint32 if b.dtype.itemsize == 4 else np.uint64)), "ladder differs"
    one = one_search()
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, batch=B, n_first=N_FIRST, max_n=MAX_N, ef=EF, ranks=RANKS, reps=REPS,
                         iters=ITERS, host_iters=HOST_ITERS, kind="f32",
                         timing="median of REPS windows, us per batch; *_wall_us: host clock around HOST_ITERS calls, each "
                                "ending with its results on the host; *_device_us: device events around ITERS launches"),
           "rungs_histogram": np.bincount(got[4], minlength=6).tolist(), "truncated": int((got[3] != 0).sum()),
           "kept_mean": float(got[2].mean()), "same_count_as_one_search": int((got[2] == one[2]).sum()),
           "rungs_launched_per_call": int(got[4].max())}
    # the cut alone, over the wide search's lists
    up = lambda a: torch.from_numpy(np.array(a if a.dtype == np.float32 else a.view(np.int32))).to(dev)
    c_ids, c_d, c_c, c_r = up(wide[0]), up(wide[1]), up(wide[2]), up(radius)
    o_ids = torch.empty((B, MAX_N), dtype=torch.int32, device=dev)
    o_d = torch.empty((B, MAX_N), dtype=torch.float32, device=dev)
    o_c, o_f = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    res["cut_device_us"], res["cut_device_us_windows"] = device_us(
        torch, lambda: H.HNSW.radius_cut_device(B, MAX_N, MAX_N, c_r, c_ids, c_d, c_c, None, o_ids, o_d, o_c, o_f, None, None, 0, stream))
    res["ladder_wall_us"], res["ladder_wall_us_windows"] = host_us(torch, ladder)
    res["one_search_wall_us"], res["one_search_wall_us_windows"] = host_us(torch, one_search)
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
