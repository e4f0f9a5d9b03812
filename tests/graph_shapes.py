"""Every search kernel on graphs no builder makes: the recipes that lay a hand-made graph over a fixture's rows, the
table of calls (one per walk routine, selected from tests/kernel_matrix.py by a rule) and the runner that holds each
call to the CPU oracle.  tests/test_gpu_graph_shapes.py runs the table on an MI355X (an environment group in a child
process of its own, `python -m tests.graph_shapes <group> [recipe ...]`); tests/test_graph_shapes_host.py checks,
without a GPU, that the recipes do what they claim.

Fixtures.  One per (kind, d, m, recipe) (`small`: per ef of the call besides, its rings are sized by it): N = 16 384
rows of H.synth_rows, imported with import_points / import_layer / set_ep into a product index and an oracle.  Nothing
is built; the oracle quantises the rows itself.  Every recipe lays its hand-made part over a deterministic background
on layer 0: the circulant graph with the eight offsets +-{1, 5, 67, 1031} (degree 8, connected).  With S0 / S1 the
index's row strides on layer 0 / above (32 / 16 at m = 16, 64 / 32 at m = 24):

  collide    C = the ids whose home bucket in a 2^12-slot visited table is one of the last three (47 ids at this N; at
             m = 24 as many of the last buckets as give S0 + 8 ids).  The top bits of the hash nest, so the same ids are
             home to the last buckets of a 2^13-slot table and of the lean kernels' quarter-size upper-layer table.  The
             members of C have level 1 and the entry point is the smallest.  A member's layer-1 row is the S1 members
             behind it (cyclically), its layer-0 row the S0 - 1 members behind it plus one background id.  One expansion
             hands a wave more ids of one bucket than the bucket and its successors to the end of the table hold: full
             buckets, the wrap past the last bucket, and the lanes of one row claiming slots of one bucket in the same
             round.  The hash constant chooses inputs only; nothing asserts on it.
  chain      one target query q*.  The ids are ordered by the oracle's own distance of this kind to q*, strictly
             decreasing (ids whose distance equals their predecessor's are left out).  Layer 2 holds the first 1 000,
             each linked to its predecessor and successor, the entry point the first; layer 1 holds those and the next
             1 000 in one chain.  Layer 0 is the background.  The greedy walk visits 1 000 ids on either upper layer:
             more than three quarters of the lean kernels' first upper table (1 024 slots), below every family's
             largest.
  degrees    hubs of degree 0, 1, S - 1, S, S + 1, S - 1 + {31, 32, 33}, S - 1 + {63, 64, 65}: on layer 0 over S0, on
             layer 1 over S1.  Every edge is symmetric, no row holds its own node.  A hub's row holds the entry point
             (id 0) and fillers of its own.  On layer 0 every node of layer 1 -- hubs and fillers -- has the entry
             point alone, and the entry point has them, layer 0's hubs and its background row: wherever the greedy walk
             ends on layer 1, layer 0 expands the entry point (a row of several hundred ids) next, and the hub whose
             stored row is the query after it.  The hubs of degree 0 stand alone (no walk reaches them).
  small      a tower: the heads of the rings alone on layers 1 .. 15 (16 layers), their rows there empty.  On layer 0
             disjoint rings of c nodes, c in {1, 2, 9, 10, 11, ef - 1, ef, ef + 1} (ef the call's), from id 0 on in
             the order ef - 1, ef, ef + 1, 1, 2, 9, 10, 11; the background holds the other ids and no edge to a ring.
             set_ep selects the ring; c = 1 is an entry point with an empty row.
  misplaced  `small` at ef 10, the entry point a node of level 0: the reference's search_layer answers
             Err("... not in Graph") on the top layer (searcher.rs:45-50).

Queries.  The base queries of KM.queries (the call's nq), then the recipe's own: `collide` the stored rows of eight
members of C; `chain` q* = base query 0 (so it is there twice) and three perturbations of it; `degrees` the hubs'
stored rows (layer 1's, then layer 0's, by degree: search_layer runs the last eight); `small` / `misplaced` the stored
rows of four ring nodes.

Table.  A walk routine is a search kernel family with its list width kept: of hx_search_kernel<KIND, P, DS, R, FAT> and
hx_filt_graph_kernel<KIND, P, DS, R> the row-shape arguments P and DS are dropped (the walk is the same code for every
row shape), every other family keeps its arguments whole.  Per routine the call ("batch" / "filtered", not of the
visited2l group) with the smallest d, then table order; the visited2l calls of that call's row on the same index; and
every "layer" and "device" call of the matrix.  "distance", "brute", "brute_fast" and "filtered_exact" walk no graph.
`layer` (search_layer on layer 0, entries 0, 3, 6) runs collide, degrees and small (one ring: the entries lie in the
first); `misplaced` runs "batch", "device" and "filtered" (search_layer has no entry point).

Runner.  KM.run_call(kernels, c, on=(idx, orc, rows, Q)), unchanged in what it asserts: the kernel log holds exactly
the row's instantiation(s) (+ `also`, + any of `may`), ids, distance bits, counts and the three counters are the
oracle's (filtered: tests/filtered_restate.py's).  A re-run after an overflow launches the call's own instantiation
and stays inside the condition; the one exception is stated in rerun_may.  `chain` pins the re-run itself where the
first table cannot hold the chain (gives_up_on_an_upper_layer).  `misplaced` has its own:
HNSW_ERR_NODE_NOT_IN_GRAPH from the call, that status for every query, counts 0, ids all ones -- where the oracle
(filtered: the restatement) raises.
"""
import os
import re
import sys

import numpy as np

from tests import kernel_matrix as KM
from tests import numeric_range as NR

N = 16384
OFFSETS = (1, 5, 67, 1031)
RECIPES = ("collide", "chain", "degrees", "small")  # (+ "misplaced", which has a runner of its own)
ALL_RECIPES = RECIPES + ("misplaced",)
CHAIN = 1000
TOWER = 15  # the level of a ring's head in `small`: 16 layers
SMALL_C = (1, 2, 9, 10, 11)
HASH = 0x9E3779B1

# ---- the table -------------------------------------------------------------------------------------------------------
# the template arguments that only shape the row fetch: dropped from a walk routine's name
ROW_SHAPE_ARGS = {"hx_search_kernel": (1, 2), "hx_filt_graph_kernel": (1, 2)}
WALK_FAMILIES = ("hx_search_kernel", "hx_search_spill_kernel", "hx_lean_q8_kernel", "hx_lean_f32_kernel",
                 "hx_pair_f32_kernel", "hx_filt_graph_kernel")
WALK_ENTRIES = ("batch", "filtered")  # (+ "layer" and "device", whose rows are taken whole)


def routine_of(kernel):
    """'hx_search_kernel<1, 25, 100, 2, false>' -> ('hx_search_kernel', '1', '2', 'false')"""
    m = re.match(r"(\w+)(?:<(.*)>)?$", kernel.strip())
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    drop = ROW_SHAPE_ARGS.get(m.group(1), ())
    return (m.group(1),) + tuple(a for i, a in enumerate(args) if i not in drop)


def selection():
    """{walk routine: (the row's kernels, its call, the visited2l calls of the same row and index)}"""
    best, order = {}, 0
    for row in KM.CASES:
        for c in row.calls:
            order += 1
            if c.entry not in WALK_ENTRIES or c.group == "visited2l":
                continue
            assert len(row.kernels) == 1, row.kernels
            key = routine_of(row.kernels[0])
            if key not in best or (c.d, order) < best[key][0]:
                best[key] = ((c.d, order), row, c)
    out = {}
    for key, (_, row, c) in best.items():
        v2l = [v for v in row.calls if v.group == "visited2l" and v.entry == c.entry and v[:4] == c[:4]]
        out[key] = (row.kernels, c, v2l)
    return out


def table():
    out = []
    for kernels, c, v2l in selection().values():
        out += [(kernels, c)] + [(kernels, v) for v in v2l]
    out += [(row.kernels, c) for row in KM.CASES for c in row.calls if c.entry in ("layer", "device")]
    return out


TABLE = table()


def recipes_of(c):
    """the recipes a call runs (module docstring)"""
    if c.entry == "layer":
        return ("collide", "degrees", "small")
    return ALL_RECIPES


def table_id(kc):
    return KM.call_id(kc[1])


# ---- graphs ----------------------------------------------------------------------------------------------------------

def strides(m):
    """(S0, S1): the slots of a layer-0 row (a power of two >= max(2m, 32)) and of an upper row (>= max(m, 8))"""
    s0, s1 = 32, 8
    while s0 < 2 * m:
        s0 *= 2
    while s1 < m:
        s1 *= 2
    return s0, s1


def home_bucket(ids, slots_log2):
    """the bucket (of four slots) a visited table of 2^slots_log2 slots looks an id up in first"""
    h = (np.asarray(ids, dtype=np.uint64) * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(32 - (slots_log2 - 2))).astype(np.int64)


def background(keep=None):
    """node -> set of neighbours: the circulant graph over the ids (keep: a bool per id, the others and every edge to
    them left out)"""
    ids = np.arange(N)
    nb = np.stack([(ids + s * o) % N for o in OFFSETS for s in (1, -1)], axis=1)
    if keep is None:
        return {int(i): set(r.tolist()) for i, r in zip(ids, nb)}
    return {int(i): set(int(x) for x in r if keep[x]) for i, r in zip(ids, nb) if keep[i]}


def link(adj, a, b):
    assert a != b
    adj[a].add(b)
    adj[b].add(a)


def isolate(adj, a):
    for b in adj[a]:
        adj[b].discard(a)
    adj[a] = set()


def csr(adj):
    nodes = sorted(adj)
    rows = [sorted(adj[n]) for n in nodes]
    offs = np.zeros(len(nodes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    flat = np.array([x for r in rows for x in r], dtype=np.uint32)
    return np.array(nodes, dtype=np.uint32), offs, flat


def degree_classes(s):
    return [0, 1, s - 1, s, s + 1] + [s - 1 + k for k in (31, 32, 33, 63, 64, 65)]


def collide_set(m):
    """C of the module docstring, ascending"""
    s0, _ = strides(m)
    b, last, k = home_bucket(np.arange(N), 12), (1 << 10) - 1, 3
    while (b > last - k).sum() < max(40, s0 + 8):
        k += 1
    return np.nonzero(b > last - k)[0]


def collide(m, dist_to):
    s0, s1 = strides(m)
    C = [int(x) for x in collide_set(m)]
    inC = set(C)
    levels = np.zeros(N, dtype=np.uint8)
    levels[C] = 1
    adj0 = background()
    adj1 = {}
    for i, c in enumerate(C):
        behind = [C[(i + k) % len(C)] for k in range(1, len(C))]
        out = min(x for x in adj0[c] if x not in inC)
        adj0[c] = set(behind[:s0 - 1]) | {out}
        adj1[c] = set(behind[:s1])
    return dict(levels=levels, layers=[adj0, adj1], ep=C[0], special=C[::len(C) // 8][:8], C=C)


def chain(m, dist_to):
    dist = dist_to(0)  # the oracle's distances of q* = base query 0 to every id
    order = np.lexsort((np.arange(N), dist))[::-1]
    keep = np.concatenate([[True], dist[order][1:] < dist[order][:-1]])
    ids = [int(x) for x in order[keep][:2 * CHAIN]]
    assert len(ids) == 2 * CHAIN
    levels = np.zeros(N, dtype=np.uint8)
    levels[ids[CHAIN:]] = 1
    levels[ids[:CHAIN]] = 2
    adj1 = {i: set() for i in ids}
    adj2 = {i: set() for i in ids[:CHAIN]}
    for a, b in zip(ids, ids[1:]):
        link(adj1, a, b)
    for a, b in zip(ids[:CHAIN], ids[1:CHAIN]):
        link(adj2, a, b)
    return dict(levels=levels, layers=[background(), adj1, adj2], ep=ids[0], special=[], chain=ids)


def degrees(m, dist_to):
    s0, s1 = strides(m)
    cls0, cls1 = degree_classes(s0), degree_classes(s1)
    perm = [int(x) for x in np.random.default_rng(0x6A5E + m).permutation(np.arange(1, N))]
    take = lambda k: [perm.pop() for _ in range(k)]
    ep, hubs1, hubs0 = 0, take(len(cls1)), take(len(cls0))
    levels = np.zeros(N, dtype=np.uint8)
    levels[[ep] + hubs1] = 1
    adj0 = background()
    adj1 = {ep: set()}
    for h in hubs1:
        adj1[h] = set()
    for h, k in zip(hubs1, cls1):
        for f in ([ep] + take(k - 1) if k else []):
            if f != ep:
                levels[f] = 1
                adj1[f] = set()
                isolate(adj0, f)
                link(adj0, f, ep)
            link(adj1, h, f)
        isolate(adj0, h)
        link(adj0, h, ep)
    for h, k in zip(hubs0, cls0):
        isolate(adj0, h)
        for f in ([ep] + take(k - 1) if k else []):
            link(adj0, h, f)
    return dict(levels=levels, layers=[adj0, adj1], ep=ep, special=hubs1 + hubs0,
                hubs=[list(zip(hubs0, cls0)), list(zip(hubs1, cls1))])


def ring_sizes(ef):
    out = []
    for c in (ef - 1, ef, ef + 1) + SMALL_C:
        if c >= 1 and c not in out:
            out.append(c)
    return out


def small(m, dist_to, ef=10):
    levels = np.zeros(N, dtype=np.uint8)
    heads, start, ring_adj = {}, 0, {}
    for c in ring_sizes(ef):
        ids = list(range(start, start + c))
        heads[c] = start
        levels[start] = TOWER
        for i in ids:
            ring_adj[i] = set()
        for a, b in zip(ids, ids[1:] + ids[:1]):
            if a != b:
                link(ring_adj, a, b)
        start += c
    keep = np.arange(N) >= start
    adj0 = background(keep)
    adj0.update(ring_adj)
    upper = [{h: set() for h in heads.values()} for _ in range(TOWER)]
    big = heads[max(heads)]
    return dict(levels=levels, layers=[adj0] + upper, ep=heads[ring_sizes(ef)[0]], heads=heads,
                special=[big, big + 1, big + 5, start + 100])


def misplaced(m, dist_to):
    g = small(m, dist_to, 10)
    g["ep"] = g["heads"][9] + 1  # a node of level 0 (the second of the ring of nine)
    return g


GRAPHS = {"collide": collide, "chain": chain, "degrees": degrees, "small": small, "misplaced": misplaced}
_FIXTURES = {}


def fixture(kind, d, m, recipe, ef=None):
    """(product index, oracle, rows, the recipe's dict: levels, layers, ep, special, ...)"""
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    key = (kind, d, m, recipe) + ((ef,) if recipe == "small" else ())
    if key not in _FIXTURES:
        rows = H.synth_rows(0, 0x6A5E0000 + d * 256 + m, 0, N, d)
        orc = O.OracleHNSW(m, 32, d, kind)
        dist_to = None
        if recipe == "chain":  # (its order needs the oracle's distances: an oracle of the points alone first)
            pts = O.OracleHNSW(m, 32, d, kind)
            pts.import_points(rows, np.zeros(N, dtype=np.uint8))
            dist_to = lambda qi: pts.distance_batch(NR.base_queries(d, qi + 1)[qi], np.arange(N, dtype=np.uint32))
        g = GRAPHS[recipe](m, dist_to, *((ef,) if recipe == "small" else ()))
        idx = H.HNSW.new(m, 32, d, kind)
        for side in (idx, orc):
            side.import_points(rows, g["levels"])
            for l, adj in enumerate(g["layers"]):
                side.import_layer(l, *csr(adj))
            side.set_ep(g["ep"])
        _FIXTURES[key] = (idx, orc, rows, g)
    return _FIXTURES[key]


def queries(c, rows, g):
    """the base queries of KM.queries (the call's nq), then the recipe's own (module docstring)"""
    base = NR.base_queries(c.d, c.nq)
    if "chain" in g:
        rng = np.random.default_rng(c.d)
        noise = rng.standard_normal((3, c.d)).astype(np.float32)
        own = np.concatenate([base[:1], base[:1] + noise * np.float32([[2.0 ** -20], [2.0 ** -10], [2.0 ** -4]])])
    else:
        own = rows[g["special"]]
    return np.concatenate([base, own]).astype(np.float32)


# ---- the runner --------------------------------------------------------------------------------------------------------

def rerun_may(kernels, c):
    """`chain` makes the lean kernels give q* up on an upper layer (HNSW_ERR_OVERFLOW) and the host run it again with
    a larger table.  The re-run is a launch of its own size: of a few queries, where the call's own launch had
    KM.MANY, so the d = 128 lean kernel takes its four-stage gather there -- the same walk routine
    but for the gather depth.  Every other re-run is the call's own instantiation."""
    if c.nq != KM.MANY:
        return ()
    return tuple(re.sub(r", 2>$", ", 4>", k) for k in kernels if k.startswith("hx_lean_f32_kernel<128,"))


# the lean and pair kernels start with a visited table of 2^12 slots up to this ef at S0 = 32 (default_slots_log2,
# search_kernels.hip) and give an upper layer a quarter of it, filled to three quarters at most: 768 ids
FIRST_TABLE_EF = 112


def gives_up_on_an_upper_layer(kernels, c):
    """`chain` visits 1 000 ids on either upper layer: a lean or pair launch with the first table must come back with
    HNSW_ERR_OVERFLOW for q* and the host (`_finish` for the device entry) run it again larger -- a second launch in
    the log, where a walk that ignored the limit would answer the same from one"""
    return c.ef <= FIRST_TABLE_EF and kernels[0].startswith(("hx_lean_", "hx_pair_"))


def run_call(kernels, c, recipe):
    """one call of the table on one recipe's fixture -> the number of KM.run_call runs (misplaced: 1)"""
    assert recipe in recipes_of(c), (recipe, c)
    if recipe == "misplaced":
        return run_misplaced(kernels, c)
    idx, orc, rows, g = fixture(c.kind, c.d, c.m, recipe, c.ef)
    Q = queries(c, rows, g)
    if recipe == "chain":
        c = c._replace(may=c.may + rerun_may(kernels, c))
    if recipe != "small":
        KM.run_call(kernels, c, on=(idx, orc, rows, Q))
        if recipe == "chain" and gives_up_on_an_upper_layer(kernels, c):
            import hnsw_rs_amd as H
            run, _ = KM._calls(c, idx, orc, rows, Q, 10)
            with H.kernel_log() as log:
                run()
            assert sum(log.values()) >= 2, ("chain %s: no re-run" % KM.call_id(c), dict(log))
        return 1
    sizes = ring_sizes(c.ef)[:1 if c.entry == "layer" else None]
    for size in sizes:
        for side in (idx, orc):
            side.set_ep(g["heads"][size])
        KM.run_call(kernels, c, on=(idx, orc, rows, Q))
    return len(sizes)


def run_misplaced(kernels, c):
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    E = H._lib.ERR_NODE_NOT_IN_GRAPH
    idx, orc, rows, g = fixture(c.kind, c.d, c.m, "misplaced")
    idx.set_option("inline_rows", c.inline)
    Q = queries(c, rows, g)
    nq = Q.shape[0]
    want = set(kernels) | set(c.also)
    for n in sorted({10, c.n}):
        what = "misplaced %s n=%d" % (KM.call_id(c), n)
        try:
            orc.search_batch(Q, n, c.ef)
        except O.OracleError as e:
            assert e.code == -3, (what, e)
        else:
            raise AssertionError("%s: the oracle answers" % what)
        if c.entry == "batch":
            run = lambda: idx.search_batch(Q, n, c.ef)[:4]
        elif c.entry == "filtered":
            from tests import filtered_restate as FR
            from tests.test_gpu_filtered import restated
            allow = np.random.default_rng(c.d * 31 + c.ef).random(N) < 0.5  # (KM._calls' mask)
            ridx = restated(idx, rows)
            for q in Q[:2]:
                try:
                    FR.graph(ridx, q, n, c.ef, lambda i: bool(allow[i]))
                except KeyError:
                    continue
                raise AssertionError("%s: the restatement answers" % what)
            idx.set_option("filter_exact_max", -1)
            run = lambda: idx.search_batch_filtered(Q, n, c.ef, allow)[:4]
        else:
            assert c.entry == "device", c
            import torch
            dev = torch.device("cuda:0")
            dQ = torch.from_numpy(Q).to(dev)
            d_ids = torch.full((nq, n), 7, dtype=torch.int32, device=dev)
            d_d = torch.zeros((nq, n), dtype=torch.float32, device=dev)
            d_c = torch.full((nq,), 7, dtype=torch.int32, device=dev)
            d_s = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
            ptrs = (dQ.data_ptr(), nq, n, c.ef, d_ids.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), 0)

            def run():
                idx.search_batch_device(*ptrs)
                idx.search_batch_device_finish(*ptrs)
                return (d_ids.cpu().numpy().view(np.uint32), d_d.cpu().numpy(), d_c.cpu().numpy().view(np.uint32),
                        d_s.cpu().numpy())
        with NR.unchecked():
            run()  # (the first call after an option change uploads the snapshot)
        with NR.unchecked() as rcs, H.kernel_log() as log:
            ids, _, counts, stats = run()
        assert [rc for rc in rcs if rc] == [E], (what, rcs)  # (the log's own calls and the enqueue return 0)
        assert want <= set(log) <= want | set(c.may), (what, dict(log))
        assert (np.asarray(stats)[:, 3].astype(np.int32) == E).all(), (what, np.asarray(stats)[:, 3])
        assert (counts == 0).all() and (ids == O.UINT32_MAX).all(), (what, counts, ids[:2])
    return 1


def main(group, recipes):
    env = KM.GROUPS[group]
    for k, v in env.items():
        assert os.environ.get(k) == v, "run group %s with %s=%s" % (group, k, v)
    calls = 0
    for recipe in (recipes or ALL_RECIPES):
        for kernels, c in TABLE:
            if c.group == group and recipe in recipes_of(c):
                run_call(kernels, c, recipe)
                calls += 1
    print("GRAPH SHAPES OK %s %d" % (group, calls))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
