"""Exact document scoring, measured.  First the union-of-pools table of scripts/late_probe.py again, on the same 20,000-row
f32 index with the labels id // 8 (2,500 documents of 8 rows) and the same 256 queries whose 4 vectors are noisy copies of
4 rows of one document: next to hnsw_search_batch_late's share of the exhaustive ten (the Chamfer ranking over ALL rows,
numpy float32 over hnsw_distance_batch of every id) among the ten returned, the share of hnsw_search_batch_late_exact at
n_cand = 16, 64 and 256 (cut to T * pool where the pools hold fewer), as pool grows.
Then, on the bench's index (1M x 100d, m 16, ef_cons 32, on-device build, as bench.py builds it) with the same labels
(125,000 documents of 8 rows), both vector kinds, 1024 queries a call, ef 64, mode sum_sq, n 10, at (T, n_in, pool) =
(4, 16, 16), (16, 64, 16) and (32, 256, 32), each figure the median of 5 after a warm-up:
  score_ms   the scoring launch alone, hnsw_score_documents_device over the n_in labels the late interaction of the
             call's own candidate lists returns, resident in HBM (device events around the one launch), with the mean
             number of documents and of scored rows a query;
  call_ms    hnsw_search_batch_late_exact with n_cand = n_in (host clock around a call that ends in a device synchronise);
  late_call_ms  hnsw_search_batch_late at the same T and pool, for the difference.

usage: python scripts/docs_probe.py OUT.json   (GPU)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hnsw_rs_amd as H  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from late_probe import (D, EF, EFC, M, N, NQ, PER_DOC, POOLS, REPS, SMALL_N, SMALL_NQ, SMALL_T, TOPN, build, events,  # noqa: E402
                        exhaustive, host_clock)  # (the recipe is scripts/late_probe.py's, so that the two tables compare)

SHAPES = ((4, 16, 16), (16, 64, 16), (32, 256, 32))  # (T, n_in, pool)
N_CANDS = (16, 64, 256)
ROWS_CAP = 4096


def share(got, want):
    return float(np.mean([np.isin(w, g).mean() for g, w in zip(got, want)]))


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
        ef = max(EF, pool)
        late = idx.search_batch_late(Q, TOPN, pool, ef, mode="sum")
        row = dict(pool=pool, ef=ef, late_share_of_the_exhaustive_ten=share(late[0], want), exact=[])
        for n_cand in N_CANDS:
            nc = max(min(n_cand, SMALL_T * pool), TOPN)
            got = idx.search_batch_late_exact(Q, TOPN, nc, pool, ef, mode="sum", rows_cap=ROWS_CAP)
            row["exact"].append(dict(n_cand=nc, share_of_the_exhaustive_ten=share(got[0], want),
                                     ten_first_documents_equal=float((got[0] == want).all(axis=1).mean())))
        out.append(row)
        print(json.dumps(row), flush=True)
    return dict(n=SMALL_N, nq=SMALL_NQ, n_vecs=SMALL_T, mode="sum", queries="4 rows of one document, noise 0.1 sigma",
                rows_cap=ROWS_CAP, by_pool=out, planted_document_is_the_exhaustive_first=float((want[:, 0] == docs).mean()))


def timings(torch, kind, name):
    dev = torch.device("cuda:0")
    idx, vs = build(N, kind)
    del vs
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = []
    for T, n_in, pool in SHAPES:
        Q = H.synth_rows(0, 0x5EED0002, 0, NQ * T, D, 16).reshape(NQ, T, D)
        d_Q = as_i32(Q)
        rows = NQ * T
        c_ids, c_dists = (torch.empty((rows, pool), dtype=torch.int32, device=dev) for _ in range(2))
        c_counts, c_stats = torch.empty(rows, dtype=torch.int32, device=dev), torch.empty((rows, 4), dtype=torch.int32, device=dev)
        idx.search_batch_device(d_Q.data_ptr(), rows, pool, EF, c_ids.data_ptr(), c_dists.data_ptr(), c_counts.data_ptr(),
                                c_stats.data_ptr(), stream)
        torch.cuda.synchronize()
        assert (c_stats.cpu().numpy()[:, 3] == 0).all(), "a query of the probe is left to _finish"
        l_labels, l_scores = (torch.empty((NQ, n_in), dtype=torch.int32, device=dev) for _ in range(2))
        l_counts = torch.empty(NQ, dtype=torch.int32, device=dev)
        idx.late_interaction_device(NQ, T, pool, n_in, "sum_sq", d_Q, c_ids, c_counts, None, l_labels, l_scores, None, None,
                                    l_counts, None, None, stream)
        o = {k: torch.empty((NQ, TOPN), dtype=torch.int32, device=dev) for k in ("labels", "scores", "best", "sizes")}
        o_counts, o_docs = (torch.empty(NQ, dtype=torch.int32, device=dev) for _ in range(2))
        score = lambda: idx.score_documents_device(NQ, T, n_in, TOPN, ROWS_CAP, "sum_sq", d_Q, l_labels, l_counts, None,  # noqa: E731
                                                   o["labels"], o["scores"], o["best"], o["sizes"], o_counts, o_docs, None, stream)
        score_ms = events(torch, score)
        mean_docs = float(o_docs.cpu().numpy().mean())
        call = lambda: idx.search_batch_late_exact(Q, TOPN, n_in, pool, EF, mode="sum_sq", rows_cap=ROWS_CAP)  # noqa: E731
        call_ms = host_clock(call)
        late_call_ms = host_clock(lambda: idx.search_batch_late(Q, TOPN, pool, EF, mode="sum_sq"))
        got = call()
        assert np.array_equal(got[0], o["labels"].cpu().numpy().view(np.uint32)), "the primitive and the call disagree"
        rows_out.append(dict(kind=name, n_vecs=T, n_in=n_in, pool=pool, score_ms=score_ms, call_ms=call_ms,
                             late_call_ms=late_call_ms, mean_documents=mean_docs, mean_scored_rows=mean_docs * PER_DOC,
                             doc_index_uploads=idx.stat("doc_index_uploads"),
                             doc_index_keys_uploaded=idx.stat("doc_index_keys_uploaded")))
        print(json.dumps(rows_out[-1]), flush=True)
    return rows_out


def main():
    import torch
    out_path = sys.argv[1]
    res = {"shape": dict(n=N, d=D, m=M, ef_cons=EFC, nq=NQ, topn=TOPN, ef=EF, mode="sum_sq", labels="id // 8", reps=REPS,
                         rows_cap=ROWS_CAP,
                         timing="medians; device events around the one launch for score_ms, host ms around a call that "
                                "ends in a device synchronise for call_ms and late_call_ms"),
           "timings": []}

    def write():
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    res["recall"] = recall()
    write()  # (kept as far as the probe got)
    for kind, name in ((H.VEC_F32, "f32"), (H.VEC_QUANT8, "quant8")):
        res["timings"] += timings(torch, kind, name)
        write()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
