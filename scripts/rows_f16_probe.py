"""The option "rows_f16" beside the plain f32 index over the SAME rows: two indexes per shape, both
by the on-device build, batch 1024, n = 10, queries and results resident in HBM (hnsw_search_batch_device, the window
ends in a device synchronise).  Shapes: 1M x 768d and 4M x 128d at efSearch 128.  The two indexes are timed alternating
in one session -- REPS windows of CALLS calls each -- and the report gives, for each, the median queries per second with
the spread of the windows, the snapshot's bytes, and recall@10 against float64 ground truth over the UNROUNDED rows
(exhaustive, on the device in float64, over the first GT_Q queries).

usage: python scripts/rows_f16_probe.py OUT.json [--quick]   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

M, EFC, B, K, EF = 16, 32, 1024, 10, 128
SHAPES = [(1_000_000, 768), (4_000_000, 128)]
REPS, CALLS, GT_Q = 7, 10, 256


def ground_truth(X, Q, dev):
    """ids of the K nearest rows of X for every query, float64 throughout, in chunks of rows"""
    q = torch.from_numpy(Q).to(dev).double()
    best_d = torch.full((len(Q), K), float("inf"), dtype=torch.float64, device=dev)
    best_i = torch.zeros((len(Q), K), dtype=torch.int64, device=dev)
    step = max(1, (1 << 27) // X.shape[1])
    for lo in range(0, len(X), step):
        x = torch.from_numpy(X[lo:lo + step]).to(dev).double()
        d2 = (x * x).sum(1)[None, :] - 2.0 * (q @ x.T)
        d, i = torch.topk(d2, min(K, d2.shape[1]), dim=1, largest=False)
        best_d, pick = torch.topk(torch.cat([best_d, d], 1), K, dim=1, largest=False)
        best_i = torch.gather(torch.cat([best_i, i + lo], 1), 1, pick)
    return best_i.cpu().numpy()


def main():
    out_path = sys.argv[1]
    shapes = [(100_000, 768), (200_000, 128)] if "--quick" in sys.argv else SHAPES
    dev = torch.device("cuda:0")
    res = {"settings": dict(m=M, ef_cons=EFC, batch=B, n=K, ef=EF, reps=REPS, calls_per_window=CALLS, gt_queries=GT_Q,
                            timing="host clock around CALLS device-pointer calls ending in a device synchronise; "
                                   "the two indexes alternate window by window in one session"),
           "shapes": []}
    for n, d in shapes:
        X = H.synth_rows(0, 0x5EED0001, 0, n, d, 16)
        Q = H.synth_rows(0, 0x5EED0002, 0, B, d, 16)
        truth = ground_truth(X, Q[:GT_Q], dev)
        dQ = torch.from_numpy(Q).to(dev)
        outs = [torch.zeros(s, dtype=t, device=dev) for s, t in
                (((B, K), torch.int32), ((B, K), torch.float32), ((B,), torch.int32), ((B, 4), torch.int32))]
        ptrs = (dQ.data_ptr(), B, K, EF) + tuple(o.data_ptr() for o in outs) + (0,)
        point = dict(n=n, d=d)
        idx = {}
        for name in ("f32", "f16"):
            ix = H.HNSW.new(M, EFC, d, H.VEC_F32)
            if name == "f16":
                ix.set_option("rows_f16", 1)
            t0 = time.perf_counter()
            ix.insert_bulk_device(X, 16, False)
            ix.upload()
            point[name + "_build_upload_s"] = time.perf_counter() - t0
            point[name + "_snapshot_bytes"] = ix.stat("snapshot_bytes")
            ix.search_batch_device(*ptrs)  # warm-up, and the answers for recall
            ix.search_batch_device_finish(*ptrs)
            ids = outs[0].cpu().numpy()[:GT_Q]
            point[name + "_recall_at_10"] = float(np.mean([len(set(a) & set(b)) for a, b in zip(ids, truth)]) / K)
            point[name + "_mean_n_dist"] = float(outs[3].cpu().numpy()[:, 0].mean())
            idx[name] = ix
        times = {"f32": [], "f16": []}
        for _ in range(REPS):
            for name in ("f32", "f16"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    idx[name].search_batch_device(*ptrs)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / CALLS)
        for name, t in times.items():
            point[name + "_qps_median"] = B / float(np.median(t))
            point[name + "_qps_min_max"] = [B / max(t), B / min(t)]
        res["shapes"].append(point)
        print(json.dumps(point), flush=True)
        del idx, X
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
