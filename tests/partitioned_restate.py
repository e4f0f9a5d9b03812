"""The merge of partitioned search (include/hnsw_mi355x.h, "partitioned search"), restated in numpy: what
hnsw_merge_topk_device, hnsw_search_batch_shards and PartitionedSearcher are held to.

Per query, over the present entries of all shards, collect (uint32 view of the distance, id_base[s] + id_stride[s] * id);
drop duplicates of the pair; sort ascending by the pair; keep n; pad the rest.  The counters are the uint32 sums over
the shards, the status that of the lowest-numbered shard whose status is not 0; a query with a merged status other than
0 gets count 0 and padded rows.  Distances are non-negative, so the order of the bits is the order of the values."""
import numpy as np

UINT32_MAX = 0xFFFFFFFF


def merge_restate(ids, dists, counts, stats, id_base, id_stride, n):
    """ids [S, nq, n] uint32 (local, pad UINT32_MAX), dists [S, nq, n] f32, counts [S, nq] or None, stats [S, nq, 4]
    (n_dist, n_exp, sum_deg, status) or None, id_base [S], id_stride [S] or None (all 1)
    -> ids [nq, n] uint32, dists [nq, n] f32, counts [nq] uint32, stats [nq, 4] int64 (None without stats)"""
    ids = np.asarray(ids).astype(np.uint32).reshape(np.shape(ids))
    S, nq, width = ids.shape
    assert width == n
    bits = np.ascontiguousarray(dists, dtype=np.float32).view(np.uint32).reshape(S, nq, n)
    base = np.asarray(id_base, dtype=np.uint64)
    stride = np.ones(S, dtype=np.uint64) if id_stride is None else np.asarray(id_stride, dtype=np.uint64)
    o_ids = np.full((nq, n), UINT32_MAX, dtype=np.uint32)
    o_bits = np.full((nq, n), np.float32(np.inf).view(np.uint32), dtype=np.uint32)
    o_counts = np.zeros(nq, dtype=np.uint32)
    o_stats = None
    if stats is not None:
        st = np.asarray(stats).astype(np.int64).reshape(S, nq, 4)
        o_stats = np.zeros((nq, 4), dtype=np.int64)
        o_stats[:, :3] = (st[:, :, :3] & 0xFFFFFFFF).sum(axis=0) & 0xFFFFFFFF
        for q in range(nq):
            failed = np.nonzero(st[:, q, 3])[0]
            o_stats[q, 3] = st[failed[0], q, 3] if failed.size else 0
    for q in range(nq):
        if o_stats is not None and o_stats[q, 3] != 0:
            continue
        keys = []
        for s in range(S):
            if counts is not None:
                present = np.arange(n) < min(int(np.asarray(counts)[s, q]) & 0xFFFFFFFF, n)
            else:
                present = ids[s, q] != UINT32_MAX
            gid = (base[s] + stride[s] * ids[s, q][present].astype(np.uint64)) & np.uint64(0xFFFFFFFF)
            keys.append((bits[s, q][present].astype(np.uint64) << np.uint64(32)) | gid)
        keys = np.unique(np.concatenate(keys))[:n]  # distinct pairs, ascending by (bits, id)
        o_counts[q] = keys.size
        o_ids[q, : keys.size] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        o_bits[q, : keys.size] = (keys >> np.uint64(32)).astype(np.uint32)
    return o_ids, o_bits.view(np.float32), o_counts, o_stats
