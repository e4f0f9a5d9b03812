"""Hybrid search on the bench's index (1M x 100d f32, m 16, ef_cons 32, on-device build, as bench.py builds it): batch
1024, n 10, pool 100, ONE external list of 100 per query (the index's own hits of a perturbed query mixed with random ids,
scores on a grid of quarters), ef 128, both modes, with and without a label range (labels 0 .. 9, the range [2, 6]).  Every
figure is the median of 5 after a warm-up, and every series is run twice, alternately, so that the two spans can be read
against each other:
  call_ms           hnsw_search_batch_hybrid (host clock around a call that ends in a device synchronise); under the range
                    at pool 64, the most a filtered candidate search returns;
  fuse_ranked_ms    the rank fusion launch alone, hnsw_fuse_ranked_device over lists resident in HBM (device events around
                    the one launch), with the distances asked for and without;
  fuse_lists_ms     the multi-vector fusion launch of multi_probe.py at T = 2, pool 100 (200 candidates), the same session;
  plain_search_ms   hnsw_search_batch of the same queries at n = 100.
What to read: the RRF launch evaluates stored rows only for its winners (and only when the distances are asked for), so
it should lie at or below the T = 2 fusion launch; the LINEAR launch evaluates every candidate once.

usage: python scripts/hybrid_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, NQ, POOL, EXT_W, TOPN, EF = 1_000_000, 100, 16, 32, 1024, 100, 100, 10, 128
REPS, ROUNDS = 5, 2
POOL_RANGED = 64
LO, HI = 2, 6


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def events(torch, fn):
    fn()
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


def main():
    import torch
    out_path = sys.argv[1]
    dev = torch.device("cuda:0")
    Q = H.synth_rows(0, 0x5EED0002, 0, NQ, D, 16)
    vs = H.synth_rows(0, 0x5EED0001, 0, N, D, 16)
    idx = H.HNSW.new(M, EFC, D, H.VEC_F32)
    t0 = time.time()
    idx.insert_bulk_device(vs, 16, False)
    idx.upload()
    del vs
    print("index built in %.1f s" % (time.time() - t0), flush=True)
    rng = np.random.default_rng(3)
    idx.set_labels(rng.integers(0, 10, N).astype(np.uint32))
    near = idx.search_batch((Q + rng.normal(0, 0.05, Q.shape)).astype(np.float32), EXT_W, EF)[0]
    ext = np.where(rng.random((NQ, EXT_W)) < 0.33, rng.integers(0, N, (NQ, EXT_W)), near).astype(np.uint32).reshape(NQ, 1, EXT_W)
    sc = np.ascontiguousarray(np.broadcast_to((np.float32(25.0) - np.float32(0.25) * np.arange(EXT_W, dtype=np.float32)),
                                              (NQ, 1, EXT_W)), dtype=np.float32)
    w = np.array([1.0, -0.05], dtype=np.float32)
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    dense = idx.search_batch(Q, POOL, EF)
    d_Q, d_ids0, d_c0, d_ext, d_sc = as_i32(Q), as_i32(dense[0]), as_i32(dense[2]), as_i32(ext), as_i32(sc)
    d_w = as_i32(np.tile(w, (NQ, 1)))
    d_lo, d_hi = as_i32(np.full(NQ, LO, dtype=np.uint32)), as_i32(np.full(NQ, HI, dtype=np.uint32))
    o_ids, o_scores, o_dists = (torch.empty((NQ, TOPN), dtype=torch.int32, device=dev) for _ in range(3))
    o_counts, o_unique, o_dropped = (torch.empty(NQ, dtype=torch.int32, device=dev) for _ in range(3))
    # multi_probe.py's fusion launch at T = 2, pool 100: the two lists of a query are the dense list and the external one
    two = np.concatenate([dense[0].reshape(NQ, 1, POOL), ext], axis=1)
    d_two, d_Q2 = as_i32(two), as_i32(np.repeat(Q[:, None, :], 2, axis=1))

    def ranked(mode, dists, ranged):
        return lambda: idx.fuse_ranked_device(NQ, mode, 60, TOPN, POOL, d_ids0, d_c0, None, 1, EXT_W, d_ext, d_sc, None, d_w, None,
                                              d_Q, o_ids, o_scores, o_dists if dists else None, o_counts, o_unique, o_dropped, None,
                                              None, None, d_lo if ranged else None, d_hi if ranged else None, stream)

    def call(mode, ranged):
        # (under a filter the candidate search is the filtered one, which returns at most 64: POOL_RANGED)
        return lambda: idx.search_batch_hybrid(Q, TOPN, POOL_RANGED if ranged else POOL, EF, ext, sc, mode=mode, weights=w,
                                               lo=LO if ranged else None, hi=HI if ranged else None)

    series = {"plain_search_ms": lambda: timed(lambda: idx.search_batch(Q, POOL, EF)),
              "fuse_lists_ms_T2_pool100": lambda: events(torch, lambda: idx.fuse_lists_device(
                  NQ, 2, POOL, TOPN, "sum", d_Q2, None, d_two, None, None, o_ids, o_scores, o_counts, o_unique, None, stream))}
    for mode in ("rrf", "linear"):
        for ranged in (False, True):
            tag = "%s%s" % (mode, "_range" if ranged else "")
            series["call_ms_" + tag] = (lambda m=mode, r=ranged: timed(call(m, r)))
            series["fuse_ranked_ms_" + tag] = (lambda m=mode, r=ranged: events(torch, ranked(m, True, r)))
        series["fuse_ranked_ms_%s_no_dists" % mode] = (lambda m=mode: events(torch, ranked(m, False, False)))
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, kind="f32", nq=NQ, pool=POOL, n_ext=1, ext_width=EXT_W, topn=TOPN, ef=EF,
                         rank_constant=60, label_range=[LO, HI], pool_of_the_ranged_calls=POOL_RANGED, reps=REPS, rounds=ROUNDS,
                         timing="medians of %d; every series run %d times alternately, both figures listed; host ms around "
                                "calls that end in a device synchronise, device events for the launches" % (REPS, ROUNDS))}
    for name in series:
        res[name] = []
    for _ in range(ROUNDS):
        for name, run in series.items():
            res[name].append(run())
    ranked("rrf", True, True)()
    torch.cuda.synchronize()
    res["mean_unique_under_the_range"] = float(o_unique.cpu().numpy().mean())
    res["mean_dropped_under_the_range"] = float(o_dropped.cpu().numpy().mean())
    ranked("rrf", True, False)()
    torch.cuda.synchronize()
    res["mean_unique"] = float(o_unique.cpu().numpy().mean())
    print(json.dumps(res), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
