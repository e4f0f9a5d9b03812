"""Diversified search on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device build, as bench.py builds it):
batch 1024, pool 64, n 10, lambda 0.5, ef 64.  Three times, each the median of 5 after a warm-up:
  call_ms        hnsw_search_batch_diverse (host clock around a call that ends in a device synchronise);
  select_ms      the selection launch alone, hnsw_diversify_device over the candidate lists resident in HBM (device
                 events around the one launch);
  host_way_ms    what a caller had before: hnsw_search_batch at n = 64, hnsw_get_vector per candidate, the pair distances
                 and the MMR loop in numpy float32 on the host (search / rows / numpy parts listed) -- whose sums are not in
                 the index's accumulation order, so its hits may differ; the share of queries with the same ids is listed.
plain_search_ms (hnsw_search_batch at n = 64) is there for scale.

usage: python scripts/diverse_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B, POOL, TOPN, EF, LAM = 1_000_000, 100, 16, 32, 1024, 64, 10, 64, 0.5
REPS = 5


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def host_way(idx, qs, parts):
    """search at n = pool, the rows one hnsw_get_vector call each, MMR in numpy float32 -> ids [B, TOPN]"""
    t0 = time.perf_counter()
    ids, dists, counts, _ = idx.search_batch(qs, POOL, EF)
    t1 = time.perf_counter()
    uniq, inv = np.unique(np.where(ids == 0xFFFFFFFF, 0, ids), return_inverse=True)  # (a pad is never read: c below)
    rows = np.stack([idx.get_point(int(i)).get_vals() for i in uniq])
    t2 = time.perf_counter()
    lam, rest = np.float32(LAM), np.float32(1.0) - np.float32(LAM)
    inv = inv.reshape(ids.shape)
    out = np.full((B, TOPN), 0xFFFFFFFF, dtype=np.uint32)
    for q in range(B):
        c = int(counts[q])
        x = rows[inv[q, :c]]
        sq = (x * x).sum(axis=1)
        pair = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - np.float32(2.0) * (x @ x.T), np.float32(0.0)))
        alive = np.ones(c, dtype=bool)
        running = np.full(c, np.inf, dtype=np.float32)
        for t in range(min(TOPN, c)):
            score = lam * dists[q, :c] - rest * (running if t else np.zeros(c, dtype=np.float32))
            score[~alive] = np.inf
            j = int(np.argmin(score))
            out[q, t] = ids[q, j]
            alive[j] = False
            running = np.minimum(running, pair[j])
    t3 = time.perf_counter()
    parts.append((t1 - t0, t2 - t1, t3 - t2))
    return out


def main():
    import torch
    out_path = sys.argv[1]
    dev = torch.device("cuda:0")
    qs = H.synth_rows(0, 0x5EED0002, 0, B, D, 16)
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    idx = H.HNSW.new(M, EFC, D, H.VEC_F32)
    t0 = time.time()
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    del vs
    print("index built in %.1f s" % (time.time() - t0), flush=True)
    plain_ms, cand = timed(lambda: idx.search_batch(qs, POOL, EF))
    call_ms, got = timed(lambda: idx.search_batch_diverse(qs, TOPN, POOL, EF, LAM))
    # the selection alone: the candidates in HBM, device events around the one launch
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    d_ids, d_dists, d_counts = as_i32(cand[0]), as_i32(cand[1]), as_i32(cand[2])
    o_ids, o_dists, o_gaps = (torch.empty((B, TOPN), dtype=torch.int32, device=dev) for _ in range(3))
    o_counts = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    select = lambda: idx.diversify_device(B, POOL, TOPN, LAM, d_ids, d_dists, d_counts, None, o_ids, o_dists, o_gaps,  # noqa: E731
                                          o_counts, None, stream)
    select()
    torch.cuda.synchronize()
    ev = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        select()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), got[0]), "the primitive and the call disagree"
    parts = []
    host_ms, host_ids = timed(lambda: host_way(idx, qs, parts))
    parts = np.median(np.array(parts[1:]), axis=0) * 1e3
    plain_top = cand[0][:, :TOPN]
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, kind="f32", batch=B, pool=POOL, topn=TOPN, ef=EF, lam=LAM, reps=REPS,
                         timing="medians; host ms around calls that end in a device synchronise, device events for select_ms"),
           "plain_search_ms": plain_ms, "call_ms": call_ms, "select_ms": float(np.median(ev)), "host_way_ms": host_ms,
           "host_way_parts_ms": dict(search=float(parts[0]), get_vector=float(parts[1]), numpy_mmr=float(parts[2])),
           "queries_whose_set_differs_from_the_plain_top": int(sum(set(a.tolist()) != set(b.tolist())
                                                                   for a, b in zip(got[0], plain_top))),
           "queries_where_the_host_way_returns_the_same_ids": int((host_ids == got[0]).all(axis=1).sum()),
           "mean_gap": float(got[2][:, 1:].mean()), "mean_dist": float(got[1].mean()),
           "mean_dist_plain_top": float(cand[1][:, :TOPN].mean())}
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
