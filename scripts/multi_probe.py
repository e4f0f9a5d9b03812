"""Multi-vector search on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device build, as bench.py builds it):
256 queries of 4 vectors, pool 32, n 10, ef 64, mode sum.  Each figure the median of 5 after a warm-up:
  call_ms          hnsw_search_batch_multi (host clock around a call that ends in a device synchronise);
  plain_search_ms  hnsw_search_batch over the same 1024 rows at n = 32, for scale (--plain-only: this figure alone, for a
                   library of the parent commit selected by HNSW_MI355X_LIB in the same session);
  fuse_ms          the fusion launch alone, hnsw_fuse_lists_device over lists resident in HBM (device events around the one
                   launch), at T * pool = 128 (4 x 32) and 256 (4 x 64);
  host_way_ms      the route a caller had before: that search, one hnsw_distance_batch per query vector over the query's
                   union of ids, and the fold in numpy (search / distance / numpy parts listed).  It computes the same
                   answer: the share of queries with the same ids and score bits is listed.

usage: python scripts/multi_probe.py OUT.json [--plain-only]   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, NQ, T, POOL, TOPN, EF = 1_000_000, 100, 16, 32, 256, 4, 32, 10, 64
REPS = 5
MAX = 0xFFFFFFFF


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), out


def host_way(idx, Q, parts):
    """search at n = pool, one distance_batch per query vector over the query's union, the fold in numpy float32"""
    t0 = time.perf_counter()
    ids, _, counts, _ = idx.search_batch(Q.reshape(NQ * T, D), POOL, EF)
    t1 = time.perf_counter()
    ids = ids.reshape(NQ, T, POOL)
    unions, dist = [], []
    for q in range(NQ):
        u = np.unique(ids[q][ids[q] != MAX])
        unions.append(u)
        dist.append([idx.distance_batch(Q[q, t], u) for t in range(T)])
    t2 = time.perf_counter()
    o_ids = np.full((NQ, TOPN), MAX, dtype=np.uint32)
    o_scores = np.full((NQ, TOPN), np.inf, dtype=np.float32)
    for q in range(NQ):
        s = dist[q][0]
        for t in range(1, T):
            s = s + dist[q][t]
        order = np.lexsort((unions[q], s))[:TOPN]
        o_ids[q, :order.size], o_scores[q, :order.size] = unions[q][order], s[order]
    t3 = time.perf_counter()
    parts.append((t1 - t0, t2 - t1, t3 - t2))
    return o_ids, o_scores


def main():
    out_path = sys.argv[1]
    plain_only = "--plain-only" in sys.argv[2:]
    Q = H.synth_rows(0, 0x5EED0002, 0, NQ * T, D, 16).reshape(NQ, T, D)
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    idx = H.HNSW.new(M, EFC, D, H.VEC_F32)
    t0 = time.time()
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    del vs
    print("index built in %.1f s" % (time.time() - t0), flush=True)
    rows = Q.reshape(NQ * T, D)
    plain_ms, cand = timed(lambda: idx.search_batch(rows, POOL, EF))
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, kind="f32", nq=NQ, n_vecs=T, pool=POOL, topn=TOPN, ef=EF, mode="sum",
                         reps=REPS, timing="medians; host ms around calls that end in a device synchronise, device events "
                                           "for fuse_ms"),
           "library": os.environ.get("HNSW_MI355X_LIB", "this commit's"), "plain_search_ms": plain_ms}
    if not plain_only:
        import torch
        dev = torch.device("cuda:0")
        call_ms, got = timed(lambda: idx.search_batch_multi(Q, TOPN, POOL, EF))
        as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
        stream = torch.cuda.current_stream().cuda_stream
        d_Q = as_i32(Q)
        fuse_ms = {}
        for pool in (POOL, 2 * POOL):
            c = cand if pool == POOL else idx.search_batch(rows, pool, EF)
            # ... and the same table size with the T lists of a query identical: the load and the dedup of T * pool
            # entries are the same work, the passes cover pool candidates instead of T * pool
            same_ids = np.repeat(c[0].reshape(NQ, T, pool)[:, :1], T, axis=1)
            same_counts = np.repeat(c[2].reshape(NQ, T)[:, :1], T, axis=1)
            for tag, l_ids, l_counts in (("", c[0], c[2]), ("_identical_lists", same_ids, same_counts)):
                d_ids, d_counts = as_i32(l_ids), as_i32(l_counts)
                o_ids, o_scores = (torch.empty((NQ, TOPN), dtype=torch.int32, device=dev) for _ in range(2))
                o_counts, o_unique = (torch.empty(NQ, dtype=torch.int32, device=dev) for _ in range(2))
                fuse = lambda: idx.fuse_lists_device(NQ, T, pool, TOPN, "sum", d_Q, None, d_ids, d_counts, None, o_ids,  # noqa: E731
                                                     o_scores, o_counts, o_unique, None, stream)
                fuse()
                torch.cuda.synchronize()
                ev = []
                for _ in range(REPS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fuse()
                    b.record()
                    torch.cuda.synchronize()
                    ev.append(a.elapsed_time(b))
                fuse_ms[str(T * pool) + tag] = float(np.median(ev))
                res["mean_unique_at_%d%s" % (T * pool, tag)] = float(o_unique.cpu().numpy().mean())
                if pool == POOL and not tag:
                    assert np.array_equal(o_ids.cpu().numpy().view(np.uint32), got[0]), "the primitive and the call disagree"
        parts = []
        host_ms, (h_ids, h_scores) = timed(lambda: host_way(idx, Q, parts))
        parts = np.median(np.array(parts[1:]), axis=0) * 1e3
        same = (h_ids == got[0]).all(axis=1) & (h_scores.view(np.uint32) == got[1].view(np.uint32)).all(axis=1)
        plain_top = cand[0].reshape(NQ, T, POOL)[:, 0, :TOPN]
        res.update({"call_ms": call_ms, "fuse_ms": fuse_ms, "host_way_ms": host_ms,
                    "host_way_parts_ms": dict(search=float(parts[0]), distance_batch=float(parts[1]), numpy_fold=float(parts[2])),
                    "queries_where_the_host_way_returns_the_same_ids_and_bits": int(same.sum()),
                    "queries_whose_set_differs_from_vector_0s_own_top": int(sum(set(a.tolist()) != set(b.tolist())
                                                                                for a, b in zip(got[0], plain_top)))})
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
