"""Late-interaction search on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds it) with
the labels id // 8 (125,000 documents of 8 rows), both vector kinds, 1024 queries a call, ef 64, mode sum_sq, n 10, at
(T, pool) = (4, 16), (16, 16) and (32, 32).  Each figure the median of 5 after a warm-up:
  search_ms   the candidate search of the call, hnsw_search_batch_device over the 1024 * T rows at n = pool (device events
              around the launch; no query of the probe needs the re-run of _finish, which is checked);
  late_ms     the late-interaction launch alone, hnsw_late_interaction_device over those lists resident in HBM (device
              events around the one launch), with the mean number of distinct candidates and of documents a query;
  call_ms     hnsw_search_batch_late (host clock around a call that ends in a device synchronise).
Then, on a 20,000-row f32 index with the same labels (2,500 documents) and 256 queries whose 4 vectors are the noisy copies of
4 rows of one document: the share of queries whose first document, and whose ten first documents, are those of the
exhaustive Chamfer ranking over ALL rows (numpy float32 over hnsw_distance_batch of every id), as pool grows, and the
mean share of the exhaustive ten that is among the ten returned.

usage: python scripts/late_probe.py OUT.json   (GPU)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402

N, D, M, EFC, NQ, TOPN, EF = 1_000_000, 100, 16, 32, 1024, 10, 64
SHAPES = ((4, 16), (16, 16), (32, 32))
SMALL_N, SMALL_NQ, SMALL_T = 20_000, 256, 4
POOLS = (4, 8, 16, 32, 64, 128, 256)
PER_DOC = 8
REPS = 5


def events(torch, fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def host_clock(fn):
    fn()  # warm-up
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def build(n, kind):
    vs = H.synth_rows(0, 0x5EED0001, 0, n, D, 16)
    idx = H.HNSW.new(M, EFC, D, kind)
    t0 = time.time()
    idx.insert_bulk_device(vs, 16, False)
    idx.set_labels((np.arange(n) // PER_DOC).astype(np.uint32))
    idx.upload()
    print("index of %d rows built in %.1f s" % (n, time.time() - t0), flush=True)
    return idx, vs


def timings(torch, kind, name):
    dev = torch.device("cuda:0")
    idx, vs = build(N, kind)
    del vs
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = []
    for T, pool in SHAPES:
        Q = H.synth_rows(0, 0x5EED0002, 0, NQ * T, D, 16).reshape(NQ, T, D)
        d_Q = as_i32(Q)
        rows = NQ * T
        c_ids, c_dists = (torch.empty((rows, pool), dtype=torch.int32, device=dev) for _ in range(2))
        c_counts, c_stats = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty((rows, 4), dtype=torch.int32, device=dev)
        search = lambda: idx.search_batch_device(d_Q.data_ptr(), rows, pool, EF, c_ids.data_ptr(), c_dists.data_ptr(),  # noqa: E731
                                                 c_counts.data_ptr(), c_stats.data_ptr(), stream)
        search_ms = events(torch, search)
        assert (c_stats.cpu().numpy()[:, 3] == 0).all(), "a query of the probe is left to _finish"
        o = {k: torch.empty((NQ, TOPN), dtype=torch.int32, device=dev) for k in ("labels", "scores", "best", "sizes")}
        o_counts, o_docs = (torch.empty(NQ, dtype=torch.int32, device=dev) for _ in range(2))
        late = lambda: idx.late_interaction_device(NQ, T, pool, TOPN, "sum_sq", d_Q, c_ids, c_counts, None, o["labels"],  # noqa: E731
                                                   o["scores"], o["best"], o["sizes"], o_counts, o_docs, None, stream)
        late_ms = events(torch, late)
        uniq = np.mean([np.unique(r).size for r in c_ids.cpu().numpy().view(np.uint32).reshape(NQ, T * pool)])
        call_ms = host_clock(lambda: idx.search_batch_late(Q, TOPN, pool, EF, mode="sum_sq"))
        got = idx.search_batch_late(Q, TOPN, pool, EF, mode="sum_sq")
        assert np.array_equal(got[0], o["labels"].cpu().numpy().view(np.uint32)), "the primitive and the call disagree"
        rows_out.append(dict(kind=name, n_vecs=T, pool=pool, search_ms=search_ms, late_ms=late_ms, call_ms=call_ms,
                             mean_distinct_candidates=float(uniq), mean_documents=float(o_docs.cpu().numpy().mean())))
        print(json.dumps(rows_out[-1]), flush=True)
    return rows_out


def exhaustive(idx, Q, n_docs):
    """the Chamfer ranking (mode sum) over ALL rows -> the ten first documents of every query"""
    all_ids = np.arange(idx.len(), dtype=np.uint32)
    top = np.zeros((Q.shape[0], TOPN), dtype=np.uint32)
    for q in range(Q.shape[0]):
        s = None
        for t in range(Q.shape[1]):
            m = idx.distance_batch(Q[q, t], all_ids).reshape(n_docs, PER_DOC).min(axis=1)
            s = m if s is None else s + m
        top[q] = np.lexsort((np.arange(n_docs), s))[:TOPN]
    return top


def recall():
    idx, vs = build(SMALL_N, H.VEC_F32)
    rng = np.random.default_rng(5)
    n_docs = SMALL_N // PER_DOC
    docs = rng.choice(n_docs, SMALL_NQ, replace=False)
    pick = np.stack([rng.choice(PER_DOC, SMALL_T, replace=False) for _ in docs])
    Q = vs[(docs[:, None] * PER_DOC + pick)] + rng.normal(0, 0.1 * vs.std(), (SMALL_NQ, SMALL_T, D)).astype(np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    want = exhaustive(idx, Q, n_docs)
    out = []
    for pool in POOLS:
        got = idx.search_batch_late(Q, TOPN, pool, max(EF, pool), mode="sum")
        out.append(dict(pool=pool, ef=max(EF, pool), first_document_equal=float((got[0][:, 0] == want[:, 0]).mean()),
                        ten_first_documents_equal=float((got[0] == want).all(axis=1).mean()),
                        mean_share_of_the_exhaustive_ten_returned=float(np.mean([np.isin(w, g).mean() for g, w in zip(got[0], want)])),
                        mean_documents=float(got[5].mean())))
        print(json.dumps(out[-1]), flush=True)
    return dict(n=SMALL_N, nq=SMALL_NQ, n_vecs=SMALL_T, mode="sum", queries="4 rows of one document, noise 0.1 sigma", by_pool=out,
                planted_document_is_the_exhaustive_first=float((want[:, 0] == docs).mean()))


def main():
    import torch
    out_path = sys.argv[1]
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, nq=NQ, topn=TOPN, ef=EF, mode="sum_sq", labels="id // 8", reps=REPS,
                         timing="medians; device events around the one launch for search_ms and late_ms, host ms around a "
                                "call that ends in a device synchronise for call_ms"),
           "timings": []}

    def write():
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for kind, name in ((H.VEC_F32, "f32"), (H.VEC_QUANT8, "quant8")):
        res["timings"] += timings(torch, kind, name)
        write()  # (kept as far as the probe got)
    res["recall"] = recall()
    write()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
