"""The lean kernels' layer-0 visited limit counts layer 0 alone: what an upper layer's table held is gone with that
table.  A hand-made graph (nothing is built): on layer 1 a chain of 600 ids in strictly decreasing order of the
oracle's distance to the query q*, so that the greedy walk visits 600 ids there -- under the 768 the upper table of a
2^12-slot launch holds; on layer 0 every row is empty but that of the chain's last node e, which has K neighbours whose
rows hold e alone.  Layer 0 then visits 1 + K ids for q*, whatever ef is.  A launch with 2^12 slots (ef <= 112 at
m = 16, default_slots_log2) takes 3 072 of them:

  K = 3 000   3 001 ids: one launch answers.  A kernel that carried the walk's count into layer 0 would see 3 601,
              give q* up with HNSW_ERR_OVERFLOW and leave it to a second, larger launch;
  K = 3 080   3 081 ids: the first launch must give up and the host run q* again -- the limit is where the test
              believes it is, from the other side.

Either way ids, distance bits, counts and the three counters are the oracle's."""
import numpy as np
import pytest

N, D, M, U = 8192, 100, 16, 600
LIMIT = 3072  # three quarters of 2^12 slots


def _graph(kind, k):
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    rows = H.synth_rows(0, 0x71A17 + kind, 0, N, D)
    q = H.synth_rows(0, 0x71A18, 0, 4, D)
    pts = O.OracleHNSW(M, 32, D, kind)
    pts.import_points(rows, np.zeros(N, dtype=np.uint8))
    dist = pts.distance_batch(q[0], np.arange(N, dtype=np.uint32))
    order = np.lexsort((np.arange(N), dist))[::-1]
    keep = np.concatenate([[True], dist[order][1:] < dist[order][:-1]])
    chain = [int(x) for x in order[keep][:U]]
    assert len(chain) == U
    inchain = set(chain)
    fillers = [i for i in range(N) if i not in inchain][:k]
    assert len(fillers) == k
    e = chain[-1]
    levels = np.zeros(N, dtype=np.uint8)
    levels[chain] = 1
    adj0 = {i: set() for i in range(N)}
    adj0[e] = set(fillers)
    for f in fillers:
        adj0[f] = {e}
    adj1 = {i: set() for i in chain}
    for a, b in zip(chain, chain[1:]):
        adj1[a].add(b)
        adj1[b].add(a)
    idx = H.HNSW.new(M, 32, D, kind)
    orc = O.OracleHNSW(M, 32, D, kind)
    for side in (idx, orc):
        side.import_points(rows, levels)
        for l, adj in enumerate((adj0, adj1)):
            nodes = sorted(adj)
            offs = np.zeros(len(nodes) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(adj[n]) for n in nodes])
            flat = np.array([x for n in nodes for x in sorted(adj[n])], dtype=np.uint32)
            side.import_layer(l, np.array(nodes, dtype=np.uint32), offs, flat)
        side.set_ep(chain[0])
    return idx, orc, q


@pytest.mark.gpu
@pytest.mark.parametrize("kind_name", ["f32", "q8"])
@pytest.mark.parametrize("k, launches", [(3000, "one"), (3080, "more")])
def test_layer0_limit_counts_layer0_alone(kind_name, k, launches):
    import hnsw_rs_amd as H
    kind = {"f32": H.VEC_F32, "q8": H.VEC_QUANT8}[kind_name]
    assert 1 + k + U > LIMIT  # (a count carried over from layer 1 would overflow either graph)
    assert (1 + k <= LIMIT) == (launches == "one")
    idx, orc, q = _graph(kind, k)
    for ef in (64, 100):  # one list register; head + tail
        idx.search_batch(q, 10, ef)  # (the first call uploads the snapshot)
        with H.kernel_log() as log:
            ids, dists, counts, stats = idx.search_batch(q, 10, ef)
        o_ids, o_d, o_c, o_s = orc.search_batch(q, 10, ef)
        lean = {name: n for name, n in log.items() if name.startswith("hx_lean_")}
        print("kind %s K %d ef %d: launches %s, n_dist of q* %d" % (kind_name, k, ef, dict(log), int(stats[0, 0])))
        assert lean, dict(log)
        assert (sum(log.values()) == 1) == (launches == "one"), (kind_name, k, ef, dict(log))
        assert np.array_equal(ids, o_ids) and np.array_equal(counts, o_c), (kind_name, k, ef)
        assert np.array_equal(dists.view(np.uint32), o_d.view(np.uint32)), (kind_name, k, ef)
        assert np.array_equal(stats[:, :3], o_s.astype(np.int64)) and (np.asarray(stats)[:, 3] == 0).all(), (kind_name, k, ef)
