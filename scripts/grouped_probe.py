"""Grouped search on one MI355X at the bench's shape (1M x 100d f32, m 16, ef_cons 32, on-device build; labels = id // 8:
125000 "documents" of eight consecutive "chunks"), batch 1024, pool 64, ef 64, n_groups 10 x per_group 3.  Three ways to
the ten nearest documents of every query:
  - search alone: hnsw_search_batch_device with n = pool (what the other two share), device events;
  - search + collapse on the device: the same launch followed by hnsw_group_by_label_device, device events;
  - search + copy-back + group_by_label on the host: the launch, the [B, pool] ids / dists / counts copied to the host
    and hnsw_rs_amd.group_by_label there over the caller's own copy of the label column -- a host clock around work
    that ends with the results on the host, against the same clock around search + collapse + the copies of the
    grouped block.
Each the median of REPS windows of ITERS back-to-back batches after a warm-up, per batch.  The three results are checked
against one another before anything is timed.

usage: python scripts/grouped_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B, POOL, EF, G, P = 1_000_000, 100, 16, 32, 1024, 64, 64, 10, 3
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
        raise SystemExit("grouped_probe needs a GPU")
    dev = torch.device("cuda:0")
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    t0 = time.time()
    index = H.HNSW.new(M, EFC, D, H.VEC_F32).insert_bulk_device(vs, 16, False)
    labels = (np.arange(N) // 8).astype(np.uint32)
    index.set_labels(labels)
    index.upload()
    print("built in %.1f s" % (time.time() - t0), flush=True)
    d_Q = torch.from_numpy(qs).to(dev)
    c_ids = torch.empty((B, POOL), dtype=torch.int32, device=dev)
    c_d = torch.empty((B, POOL), dtype=torch.float32, device=dev)
    c_c = torch.empty(B, dtype=torch.int32, device=dev)
    c_st = torch.empty((B, 4), dtype=torch.int32, device=dev)
    o_ids = torch.empty((B, G, P), dtype=torch.int32, device=dev)
    o_d = torch.empty((B, G, P), dtype=torch.float32, device=dev)
    o_lab = torch.empty((B, G), dtype=torch.int32, device=dev)
    o_sz = torch.empty((B, G), dtype=torch.int32, device=dev)
    o_c = torch.empty(B, dtype=torch.int32, device=dev)
    o_st = torch.empty((B, 4), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def search():
        index.search_batch_device(d_Q.data_ptr(), B, POOL, EF, c_ids.data_ptr(), c_d.data_ptr(), c_c.data_ptr(),
                                  c_st.data_ptr(), stream)

    def collapse():
        index.group_by_label_device(B, POOL, G, P, c_ids, c_d, c_c, c_st, o_ids, o_d, o_lab, o_sz, o_c, o_st, stream)

    def search_collapse():
        search()
        collapse()

    def device_way():
        search_collapse()
        return [t.cpu().numpy() for t in (o_ids, o_d, o_lab, o_sz, o_c)]

    def host_way():
        search()
        ids, dists, counts = c_ids.cpu().numpy().view(np.uint32), c_d.cpu().numpy(), c_c.cpu().numpy().view(np.uint32)
        # (the caller's own copy of the column stands in for hnsw_get_labels: the cheaper of the two for the host)
        return H.group_by_label(ids, dists, counts, labels, G, P)

    # the three agree before anything is timed
    got_dev = device_way()
    got_host = host_way()
    whole = index.search_batch_grouped(qs, G, P, POOL, EF)
    assert int((c_st[:, 3] != 0).sum()) == 0, "a query did not finish with status 0"
    for a, b, c in zip(got_dev, got_host, whole):
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), "device and host collapse differ"
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(c).view(np.uint32)), "primitive and entry point differ"
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, batch=B, pool=POOL, ef=EF, n_groups=G, per_group=P, reps=REPS,
                         iters=ITERS, host_iters=HOST_ITERS, kind="f32", labels="id // 8",
                         timing="median of REPS windows, us per batch; *_device_us: device events around ITERS back-to-back "
                                "batches; *_wall_us: host clock around HOST_ITERS batches, each ending with its results on the host"),
           "groups_found_mean": float(got_dev[4].mean())}
    res["search_device_us"], res["search_device_us_windows"] = device_us(torch, search)
    res["search_collapse_device_us"], res["search_collapse_device_us_windows"] = device_us(torch, search_collapse)
    res["collapse_device_us"], res["collapse_device_us_windows"] = device_us(torch, collapse)
    res["device_way_wall_us"], res["device_way_wall_us_windows"] = host_us(torch, device_way)
    res["host_way_wall_us"], res["host_way_wall_us_windows"] = host_us(torch, host_way)
    res["entry_point_wall_us"], res["entry_point_wall_us_windows"] = host_us(
        torch, lambda: index.search_batch_grouped(qs, G, P, POOL, EF))
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
