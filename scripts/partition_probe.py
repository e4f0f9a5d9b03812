"""Partitioned search on one MI355X: the bench's points (1M x 100d f32, m 16, ef_cons 32, on-device build) cut into
S in {1, 2, 4, 8} contiguous shards on the one GPU.  Per S, at n = 10 and ef = 64, batch 1024:
  - recall@10 of PartitionedIndex.search_batch against hnsw_brute_force over the unsplit points;
  - the summed shard-search kernel time: device events around the S hnsw_search_batch_device launches of one batch;
  - the merge kernel time: device events around hnsw_merge_topk_device over the S lists;
each the median of REPS windows of ITERS back-to-back batches after a warm-up, per batch; and the merge's share of the
two.  S = 1 is the unsplit index plus a one-list merge.

usage: python scripts/partition_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
from hnsw_rs_amd.partitioned import partition_rows  # noqa: E402

N, D, M, EFC, B, TOPN, EF = 1_000_000, 100, 16, 32, 1024, 10, 64
SHARDS = [1, 2, 4, 8]
REPS, ITERS = 5, 100


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


def main():
    import torch
    out_path = sys.argv[1]
    if H.device_count() < 1:
        raise SystemExit("partition_probe needs a GPU")
    dev = torch.device("cuda:0")
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, batch=B, topn=TOPN, ef=EF, reps=REPS, iters=ITERS, kind="f32",
                         timing="device events around ITERS back-to-back batches, median of REPS windows, us per batch"),
           "points": []}
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    d_Q = torch.from_numpy(qs).to(dev)
    gt = None
    for S in SHARDS:
        rows, base, stride = partition_rows(N, S, "contiguous")
        t0 = time.time()
        shards = [H.HNSW.new(M, EFC, D, H.VEC_F32).insert_bulk_device(vs[r], 16, False) for r in rows]
        for s in shards:
            s.upload()
        p = H.PartitionedIndex(shards, base, stride, "contiguous", N)
        print("S=%d built in %.1f s" % (S, time.time() - t0), flush=True)
        if gt is None:
            gt, _ = shards[0].brute_force(qs, TOPN)  # (S = 1 comes first: the unsplit index)
        ids, _, counts, _ = p.search_batch(qs, TOPN, EF)
        hits = sum(len(set(a[:c].tolist()) & set(b.tolist())) for a, c, b in zip(ids, counts, gt))
        l_ids = torch.empty((S, B, TOPN), dtype=torch.int32, device=dev)
        l_d = torch.empty((S, B, TOPN), dtype=torch.float32, device=dev)
        l_c = torch.empty((S, B), dtype=torch.int32, device=dev)
        l_st = torch.empty((S, B, 4), dtype=torch.int32, device=dev)
        o_ids = torch.empty((B, TOPN), dtype=torch.int32, device=dev)
        o_d = torch.empty((B, TOPN), dtype=torch.float32, device=dev)
        o_c = torch.empty(B, dtype=torch.int32, device=dev)
        o_st = torch.empty((B, 4), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def search():
            for k, s in enumerate(shards):
                s.search_batch_device(d_Q.data_ptr(), B, TOPN, EF, l_ids[k].data_ptr(), l_d[k].data_ptr(),
                                      l_c[k].data_ptr(), l_st[k].data_ptr(), stream)

        def merge():
            H.merge_topk(S, B, TOPN, l_ids, l_d, l_c, l_st, base, stride, o_ids, o_d, o_c, o_st, stream)

        search_us, search_all = window_us(torch, search)
        merge_us, merge_all = window_us(torch, merge)
        assert int((l_st[:, :, 3] != 0).sum()) == 0, "a shard query did not finish with status 0"
        assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), ids), "the timed merge differs from search_batch"
        pt = dict(shards=S, recall10=hits / (B * TOPN), search_us=search_us, search_us_windows=search_all,
                  merge_us=merge_us, merge_us_windows=merge_all, merge_share=merge_us / (merge_us + search_us))
        res["points"].append(pt)
        print(json.dumps(pt), flush=True)
        del p, shards
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
