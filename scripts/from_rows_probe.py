"""Search from stored rows on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device build, as bench.py builds it):
batch 1024 sources, n 10, ef 64.  Each time is the median of 5 after a warm-up:
  by_id_ms         hnsw_search_batch_by_id (host clock around a call that ends in a device synchronise);
  plain_search_ms  hnsw_search_batch at n = 11 on the same rows already on the host, for scale;
  compose_ms       the compose launch alone, hnsw_compose_rows_device (device events around the one launch);
  drop_ms          the drop launch alone, hnsw_drop_ids_device over the candidate lists resident in HBM (device events);
  from_rows_w8_ms  hnsw_search_batch_from_rows at width 8 with weights;
  host_way_ms      what a caller had before: hnsw_get_vector per id through the binding, hnsw_search_batch at n + 1, the
                   drop of the source in numpy (get_vector / search / numpy parts listed).

usage: python scripts/from_rows_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, B, TOPN, EF, WIDTH = 1_000_000, 100, 16, 32, 1024, 10, 64, 8
REPS = 5


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def events(torch, fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    ev = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    return float(np.median(ev))


def host_way(idx, src, parts):
    """the rows one hnsw_get_vector call each, search at n + 1, the source taken out on the host -> ids [B, TOPN]"""
    t0 = time.perf_counter()
    rows = np.stack([idx.get_point(int(i)).get_vals() for i in src])
    t1 = time.perf_counter()
    ids, dists, counts, _ = idx.search_batch(rows, TOPN + 1, EF)
    t2 = time.perf_counter()
    out = np.full((B, TOPN), 0xFFFFFFFF, dtype=np.uint32)
    for q in range(B):
        keep = ids[q, :int(counts[q])]
        keep = keep[keep != src[q]][:TOPN]
        out[q, :keep.size] = keep
    t3 = time.perf_counter()
    parts.append((t1 - t0, t2 - t1, t3 - t2))
    return out


def main():
    import torch
    out_path = sys.argv[1]
    dev = torch.device("cuda:0")
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    idx = H.HNSW.new(M, EFC, D, H.VEC_F32)
    t0 = time.time()
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    print("index built in %.1f s" % (time.time() - t0), flush=True)
    rng = np.random.default_rng(5)
    src = rng.choice(N, B, replace=False).astype(np.uint32)
    rows = np.ascontiguousarray(vs[src])
    del vs
    plain_ms, cand = timed(lambda: idx.search_batch(rows, TOPN + 1, EF))
    by_id_ms, got = timed(lambda: idx.search_batch_by_id(src, TOPN, EF))
    src8 = rng.integers(0, N, (B, WIDTH)).astype(np.uint32)
    src8[:, 0] = src
    w8 = rng.random((B, WIDTH), dtype=np.float32)
    w8_ms, _ = timed(lambda: idx.search_batch_from_rows(src8, w8, TOPN, EF))
    # the two launches alone: everything in HBM, device events around the one launch
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    d_src, d_src8, d_w8 = as_i32(src), as_i32(src8), as_i32(w8)
    d_Q = torch.empty((B, D), dtype=torch.float32, device=dev)
    compose_ms = events(torch, lambda: idx.compose_rows_device(B, 1, d_src, None, d_Q, None, stream))
    assert np.array_equal(d_Q.cpu().numpy().view(np.uint32), rows.view(np.uint32)), "the composed rows are not the stored rows"
    compose8_ms = events(torch, lambda: idx.compose_rows_device(B, WIDTH, d_src8, d_w8, d_Q, None, stream))
    d_ids, d_dists, d_counts = as_i32(cand[0]), as_i32(cand[1]), as_i32(cand[2])
    o_ids, o_dists = (torch.empty((B, TOPN), dtype=torch.int32, device=dev) for _ in range(2))
    o_counts = torch.empty(B, dtype=torch.int32, device=dev)
    drop_ms = events(torch, lambda: H.HNSW.drop_ids_device(B, TOPN + 1, TOPN, 1, d_src, None, d_ids, d_dists, d_counts, None,
                                                           o_ids, o_dists, o_counts, None, None, stream))
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), got[0]), "the primitive and the call disagree"
    parts = []
    host_ms, host_ids = timed(lambda: host_way(idx, src, parts))
    parts = np.median(np.array(parts[1:]), axis=0) * 1e3
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, kind="f32", batch=B, topn=TOPN, ef=EF, width=WIDTH, reps=REPS,
                         timing="medians; host ms around calls that end in a device synchronise, device events for "
                                "compose_ms and drop_ms"),
           "by_id_ms": by_id_ms, "plain_search_ms": plain_ms, "compose_ms": compose_ms, "compose_w8_ms": compose8_ms,
           "drop_ms": drop_ms, "from_rows_w8_ms": w8_ms, "host_way_ms": host_ms,
           "host_way_parts_ms": dict(get_vector=float(parts[0]), search=float(parts[1]), numpy_drop=float(parts[2])),
           "queries_where_the_host_way_returns_the_same_ids": int((host_ids == got[0]).all(axis=1).sum()),
           "queries_whose_source_was_in_its_list": int((np.asarray(cand[0]) == src[:, None]).any(axis=1).sum())}
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
