"""(test infrastructure: uses the oracle's restatement; run from the repo root)
Design simulation: the runner-up's misses in the lean f32 kernel's two-row pass (search_lean.hip, layer 0).

A pass picks the two smallest unexpanded entries of the list, c and p, expands c, merges c's fresh keys and commits p
from the registers when p is still the smallest unexpanded entry (a hit).  It is not (a miss) exactly when a fresh key
of c lies below p's key, and then the next pick is known before the merge: its candidate is the smallest such key, its
runner-up the second smallest or -- there being only one -- p again, unless the merge pushed that entry off the list
(p when the merge fills the list; the second smallest key only where p was the list's last entry).  `replay`
restates the pass over any distance function and records every pass; tests/test_runner_up_miss_host.py holds the rule
to it, tests/test_gpu_runner_up_miss.py proves its hand-made graphs with it.

    python tests/tools/miss_sim.py [N] [ef] [queries]

Expected output (N = 1 000 000 x 100d recipe A, host-built, M = 16, ef_construction = 32, efSearch 68, 320 bench
queries; per query, mean | the slowest 5 % by passes):

    layer-0 passes                                   39.3 | 44.9
    hits (p committed)                               29.6 | 26.1
    misses                                            8.1 | 16.9
    misses with 1 / 2 / >= 3 fresh keys below p       5.6 / 1.3 / 1.2 | 12.4 / 2.5 / 2.1
    next pick predicted correctly                    8.07 of 8.11 | 16.75 of 16.94
    next pass's runner-up is the old p                5.6 | 12.3

The host build races its eight threads, so the graph and with it every figure moves by a few tenths from run to run
(another run: 39.5 | 46.4, 29.3 | 25.2, 8.4 | 18.9, 5.8 / 1.4 / 1.2 | 13.3 / 3.8 / 1.8, 8.41 of 8.43 | 18.69 of 18.88,
5.8 | 13.1).  The stamps build counts the same on the GPU for the graph the bench runs (scripts/stamps_lean.py,
profiles/runner_up_miss.txt: 39.4 passes, 8.4 misses, 5.7 / 1.5 / 1.2, 8.33 predicted, 5.6 with p again).
"""
import bisect
import sys


def replay(adj0, dist_of, entry, ef, s0=32):
    """The two-row pass on layer 0.  adj0: node -> sequence of neighbour ids; dist_of(ids) -> their distances to the
    query (float32); entry: the (distance, id) key layer 0 starts from; s0: slots of a stored layer-0 row (a row of
    more neighbours carries an overflow pointer: as c it takes passes of its own, as p it is not speculated on).
    -> (the list: ascending (distance, id) keys, (n_dist, n_exp, sum_deg) of layer 0, passes).  A pass is a dict:
    c, p (ids; p None without a runner-up), ordinary (both rows within s0), hit, below (the fresh keys of c below
    p's key, ascending; [] without p), p_left (p fell off the list in c's merge), second_left (so did the second
    smallest of `below`: p was the list's last entry and the list is full)."""
    ef = max(1, ef)
    sel, expanded, visited = [entry], set(), {entry[1]}
    counters = [0, 0, 0]

    def unexp(k):
        out = []
        for e in sel:
            if e[1] not in expanded:
                out.append(e)
                if len(out) == k:
                    break
        return out

    def expand(node):
        expanded.add(node)
        nbrs = [int(x) for x in adj0[node]]
        fresh = [n for n in nbrs if n not in visited]
        fresh = list(dict.fromkeys(fresh))
        visited.update(fresh)
        counters[0] += len(fresh)
        counters[1] += 1
        counters[2] += len(nbrs)
        if not fresh:
            return []
        ds = dist_of(fresh)
        for d in ds:
            if d != d:
                raise ValueError("NaN distance")
        return [(float(d), n) for d, n in zip(ds, fresh)]

    def merge(keys):
        for k in keys:
            bisect.insort(sel, k)
        del sel[ef:]

    passes = []
    while True:
        u = unexp(2)
        if not u:
            break
        c = u[0]
        p = u[1] if len(u) > 1 else None
        ordinary = p is not None and len(adj0[c[1]]) <= s0 and len(adj0[p[1]]) <= s0
        keys = expand(c[1])
        below = sorted(k for k in keys if p is not None and k < p)
        merge(keys)
        rec = dict(c=c[1], p=None if p is None else p[1], ordinary=ordinary, hit=False, below=below,
                   p_left=p is not None and p not in sel, second_left=len(below) > 1 and below[1] not in sel)
        passes.append(rec)
        if not ordinary:
            continue
        nxt = unexp(1)
        if nxt and nxt[0] == p:
            assert not below
            rec["hit"] = True
            merge(expand(p[1]))
        else:
            assert below, "a miss without a fresh key below the runner-up"
    return sel, tuple(counters), passes


def predicted(rec):
    """the pair a miss foresees for the next pick: (candidate, runner-up)"""
    b = rec["below"]
    return b[0][1], (b[1][1] if len(b) > 1 else rec["p"])


def tally(passes):
    """per-query counts of the expected output: passes, hits, misses, misses by keys below p (1, 2, >= 3), follow-up
    picks predicted, follow-up passes whose runner-up is the old p"""
    t = dict(passes=len(passes), hits=0, misses=0, b1=0, b2=0, b3=0, predicted=0, old_p_again=0)
    for i, r in enumerate(passes):
        if not r["ordinary"]:
            continue
        if r["hit"]:
            t["hits"] += 1
            continue
        t["misses"] += 1
        t["b%d" % min(3, len(r["below"]))] += 1
        if i + 1 < len(passes):
            nx = passes[i + 1]
            t["predicted"] += (nx["c"], nx["p"]) == predicted(r)
            t["old_p_again"] += nx["p"] == r["p"]
    return t


def main(argv):
    sys.path.insert(0, ".")
    import time
    import numpy as np
    import hnsw_rs_amd as H
    from oracle import restate_np as R
    N = int(argv[1]) if len(argv) > 1 else 1000000
    ef = int(argv[2]) if len(argv) > 2 else 68
    nq = int(argv[3]) if len(argv) > 3 else 320
    d = 100
    vs = H.synth_rows(0, 0x5EED0001, 0, N, d, 8)
    qs = H.synth_rows(0, 0x5EED0002, 0, nq, d, 1)
    t = time.time()
    idx = H.HNSW.new(16, 32, d, H.VEC_F32).insert_bulk(vs, 8, False)
    print("build %.0fs" % (time.time() - t))
    csr = [idx.get_layer(l).csr() for l in range(idx.nb_layers())]
    ri = R.Index.from_csr(vs, R.VEC_F32, csr, int(idx.params.ep))
    rows = []
    for q in qs:
        point = ri.point(q)
        r = R.Results()
        r.selected.add(R._key(ri.dists([ri.ep], point)[0], ri.ep))
        for l in range(len(ri.layers) - 1, 0, -1):
            R.search_layer(ri, r, ri.layers[l], point, 1)
        _, _, passes = replay(ri.layers[0], lambda ids: ri.dists(ids, point), r.selected[0], ef)
        rows.append(tally(passes))
    keys = ("passes", "hits", "misses", "b1", "b2", "b3", "predicted", "old_p_again")
    T = np.array([[r[k] for k in keys] for r in rows], dtype=np.float64)
    slow = np.argsort(-T[:, 0])[:max(1, nq // 20)]
    m, s = T.mean(0), T[slow].mean(0)
    print("layer-0 passes                                   %.1f | %.1f" % (m[0], s[0]))
    print("hits (p committed)                               %.1f | %.1f" % (m[1], s[1]))
    print("misses                                            %.1f | %.1f" % (m[2], s[2]))
    print("misses with 1 / 2 / >= 3 fresh keys below p       %.1f / %.1f / %.1f | %.1f / %.1f / %.1f" % (
        m[3], m[4], m[5], s[3], s[4], s[5]))
    print("next pick predicted correctly                    %.2f of %.2f | %.2f of %.2f" % (m[6], m[2], s[6], s[2]))
    print("next pass's runner-up is the old p                %.1f | %.1f" % (m[7], s[7]))


if __name__ == "__main__":
    main(sys.argv)
