"""The runner-up's misses in the lean f32 kernel's two-row pass (search_lean.hip): the fixtures and the
CPU replay glue of tests/test_runner_up_miss_host.py (no GPU) and tests/test_gpu_runner_up_miss.py.

Built index.  20 000 rows of H.synth_rows at d = 100, f32, M = 16, ef_construction = 32, built on the host by the
oracle's batch-synchronous insert (the same graph wherever it runs, whatever the thread count) and imported into the
product.  256 queries.

Hand-made layer-0 graphs.  One layer, N = 8 192 ids of which a few hundred take part (the visited table's hash spreads
consecutive ids over its 1 024 buckets, so ids that share a home bucket -- `stale` needs five -- are thousands apart);
the others have empty rows and are never reached.  The target query q* is the origin and row i is (r_i, 0, ..., 0):
its distance to q* is r_i exactly (integers up to 4 096: the square is exact in f32, the other 99 terms are zero, the
root of an exact square is exact).  Every graph starts at an entry point e whose row holds the first candidate and a
runner-up P; what a graph's name promises is asserted on the replay's passes (assert_pattern) before anything is asked
of a GPU.  With (c, p) a pass's candidate and runner-up:

  one      x_j -> x_j+1, every x below P: 43 passes in a row miss with one key below P and keep P, then P is committed
  two      every candidate's row holds two new ids below the runner-up: 40 misses with two keys, the pair predicted
  five     ... five new ids (the merge goes through LDS): 40 misses with five keys
  stale    `one`, and the candidates in between insert into the buckets P's lanes looked at: one of P's neighbours
           itself (slot now holds the id), an id of the same home bucket (slot taken by another id), four of them
           (home bucket full); a fourth neighbour's bucket stays as it was (slot still empty)
  falls    rows of one, one and two new ids in turn, every id below all before it: at ef 2 every miss pushes its
           runner-up off the list, at ef 3 a runner-up is kept once and pushed off by the next miss; the row of two
           then gives the walk a new pair
  overflow `one` where every fourth x has 40 neighbours (degree > S0: the foreseen candidate's row carries the overflow
           pointer), then the same under a runner-up whose own row does (not speculated on)
  ties     every distance of the walk is P's; ids below P's sort below it, ids above do not: one tie below and one
           above per pass, then two ties below per pass
"""
import numpy as np

from tests import graph_shapes as GS
from tests.tools import miss_sim

D, M, S0 = 100, 16, 32
EFS = (1, 2, 3, 10, 64, 68, 128, 129, 256)
N_BUILT, NQ_BUILT = 20000, 256
N = 8192
FAR = 4096.0
TOPN = 10

_CACHE = {}


# ---- the built index -------------------------------------------------------------------------------------------------

def built():
    """(oracle, rows, levels, queries) of the built index"""
    if "built" not in _CACHE:
        import hnsw_rs_amd as H
        from oracle import oracle_py as O
        vs = H.synth_rows(0, 0x5EED0001, 0, N_BUILT, D)
        qs = H.synth_rows(0, 0x5EED0002, 0, NQ_BUILT, D)
        lv = O.draw_levels(N_BUILT, M, 0x5EED0003)
        orc = O.OracleHNSW(M, 32, D, O.VEC_F32)
        orc.insert_bulk_batched(vs, lv, nthreads=8)
        _CACHE["built"] = (orc, vs, lv, qs)
    return _CACHE["built"]


def layer0(orc):
    ids, offs, nbrs = orc.layer_csr(0)
    return {int(n): nbrs[int(offs[i]):int(offs[i + 1])].tolist() for i, n in enumerate(ids)}


def entry_of(orc, q):
    """the (distance, id) key layer 0 starts from: the greedy walk down the upper layers"""
    cur = orc.ep
    for l in range(orc.nb_layers - 1, 0, -1):
        cur = int(orc.search_layer(l, q, [cur], 1)[0][0])
    return float(orc.distance_batch(q, [cur])[0]), cur


def replay(orc, adj0, q, ef):
    """tests/tools/miss_sim.replay over the oracle's distances -> (list, layer-0 counters, passes)"""
    dist = orc.distance_batch(q, np.arange(len(orc), dtype=np.uint32))
    return miss_sim.replay(adj0, lambda ids: dist[ids], entry_of(orc, q), ef, S0)


def check_rule(passes, what=""):
    """The rule the kernel's foresight rests on: whenever a fresh key of c lies below p's key, the next pick's candidate
    is the smallest such key (it always survives the merge: it takes p's place or one before it) and its runner-up the
    second smallest -- or, there being one only, the old p -- unless that entry has left the list (the second smallest
    can only where p was the list's last entry).  -> the number of passes it was checked on"""
    n = 0
    for i, r in enumerate(passes):
        if not r["below"]:
            continue
        assert i + 1 < len(passes), (what, "a fresh key below the runner-up and no pass after it", r)
        nx, b = passes[i + 1], r["below"]
        assert nx["c"] == b[0][1], (what, i, r, nx)
        if len(b) > 1 and r["second_left"]:
            assert r["p_left"] and nx["p"] not in (b[1][1], r["p"]), (what, i, r, nx)
        elif len(b) > 1:
            assert nx["p"] == b[1][1], (what, i, r, nx)
        elif r["p_left"]:
            assert nx["p"] != r["p"], (what, i, r, nx)
        else:
            assert nx["p"] == r["p"], (what, i, r, nx)
        n += 1
    return n


# ---- hand-made graphs ------------------------------------------------------------------------------------------------

class Graph:
    def __init__(self, seed):
        self.adj = {i: [] for i in range(N)}
        self.r = np.full(N, FAR, dtype=np.float32)
        self.used = set()
        self.pool = [int(x) for x in np.random.default_rng(seed).permutation(N)]
        self.info = {}

    def node(self, radius, id=None):
        if id is None:
            id = next(x for x in self.pool if x not in self.used)
        assert id not in self.used and 0 < radius < FAR
        self.used.add(id)
        self.r[id] = radius
        return id

    def edge(self, a, b):
        assert a != b and b not in self.adj[a]
        self.adj[a].append(b)

    def start(self, first_r, p_r, p_id=None, first_id=None):
        """e -> {the first candidate, P}"""
        e, P, x = self.node(3000), self.node(p_r, p_id), self.node(first_r, first_id)
        self.edge(e, P)
        self.edge(e, x)
        self.ep = e
        return P, x


def g_one(length=44):
    g = Graph(1)
    P, x = g.start(999, 1000)
    for j in range(1, length):
        nx = g.node(999 - j)
        g.edge(x, nx)
        x = nx
    for j in range(20):
        g.edge(P, g.node(2000 + j))
    g.info = dict(P=P)
    return g


def g_many(k, levels=42):
    """every candidate's row: k new ids, all below the runner-up"""
    g = Graph(2 + k)
    P, x = g.start(999, 1000)
    for j in range(20):
        g.edge(P, g.node(2000 + j))
    for j in range(1, levels + 1):
        level = [g.node(900 - k * j - k + i) for i in range(1, k + 1)]  # ascending; all below the level before
        for y in level:
            g.edge(x, y)
        x = level[0]
    return g


def same_bucket(g, count):
    """`count` unused ids of one home bucket of the lean kernels' first table (2^12 slots) that holds no used id"""
    b = GS.home_bucket(np.arange(N), 12)
    taken = {int(b[i]) for i in g.used}
    for bucket in range(1 << 10):
        ids = [int(i) for i in np.nonzero(b == bucket)[0]]
        if bucket not in taken and len(ids) >= count:
            return ids[:count]
    raise AssertionError("no bucket with %d unused ids" % count)


def g_stale():
    g = Graph(11)
    P, x = g.start(999, 1000)
    chain = [x]
    for j in range(1, 12):
        nx = g.node(999 - j)
        g.edge(x, nx)
        chain.append(nx)
        x = nx
    two = same_bucket(g, 2)
    y_taken, z_other = g.node(2001, two[0]), g.node(2101, two[1])
    five = same_bucket(g, 5)
    y_full = g.node(2002, five[0])
    z_full = [g.node(2102 + i, five[1 + i]) for i in range(4)]
    y_same, y_empty = g.node(2003), g.node(2004)
    for y in (y_taken, y_full, y_same, y_empty):
        g.edge(P, y)
    for j in range(12):
        g.edge(P, g.node(2010 + j))
    g.edge(chain[2], z_other)  # a slot P's lanes saw empty is taken by another id
    g.edge(chain[4], y_same)   # ... now holds the id itself
    for z in z_full:           # ... and a home bucket fills up
        g.edge(chain[6], z)
    hb = lambda i: int(GS.home_bucket([i], 12)[0])
    assert hb(y_taken) == hb(z_other) and all(hb(z) == hb(y_full) for z in z_full)
    assert len({hb(y_taken), hb(y_full), hb(y_same), hb(y_empty)}) == 4
    g.info = dict(P=P, chain=chain)
    return g


def g_falls(cycles=12):
    """rows of one, one and two new ids in turn, every id below all before it: (c, p) -> k1 -> k2 -> (c', p')"""
    g = Graph(12)
    P, x = g.start(999, 1000)
    r = 999
    for _ in range(cycles):
        k1, k2, b, a = (g.node(r - i) for i in (1, 2, 3, 4))
        g.edge(x, k1)
        g.edge(k1, k2)
        g.edge(k2, a)
        g.edge(k2, b)
        x, r = a, r - 4
    return g


def g_overflow(length=24):
    g = Graph(13)
    P, x = g.start(999, 1000)
    fat = []
    for j in range(1, length):
        nx = g.node(999 - j)
        g.edge(x, nx)
        if j % 4 == 0:
            for i in range(40):
                g.edge(nx, g.node(3100 + (j * 40 + i) % 900))
            fat.append(nx)
        x = nx
    # ... then a runner-up P2 whose own row overflows, under a second stretch of the chain
    P2 = g.node(950 - length)
    g.edge(x, P2)
    for i in range(40):
        g.edge(P2, g.node(3050 + i % 40))
    for j in range(8):
        nx = g.node(940 - length - j)
        g.edge(x, nx)
        x = nx
    g.info = dict(fat=fat, P2=P2)
    return g


def g_ties(pairs, length=24):
    """pairs False: per pass one id below P's and one above, all at P's distance; True: two below"""
    g = Graph(14 + pairs)
    pid = 4000
    below = iter(range(pid - 1, 0, -1))   # descending: every new id sorts below every runner-up before it
    above = iter(range(pid + 1, N))
    take = lambda it: next(i for i in it if i not in g.used)
    P, x = g.start(1000, 1000, p_id=pid, first_id=take(below))
    for j in range(12):
        g.edge(P, g.node(2000 + j))
    for j in range(length):
        if pairs:
            hi, lo = take(below), take(below)
            g.edge(x, g.node(1000, hi))
            g.edge(x, g.node(1000, lo))
            x = lo
        else:
            nx = g.node(1000, take(below))
            g.edge(x, nx)
            g.edge(x, g.node(1000, take(above)))
            x = nx
    g.info = dict(P=P)
    return g


GRAPHS = {
    "one": (g_one, (64, 68, 129)),
    "two": (lambda: g_many(2), (64, 68, 129)),
    "five": (lambda: g_many(5), (64, 68, 129)),
    "stale": (g_stale, (64, 68)),
    "falls": (g_falls, (2, 3)),
    "overflow": (g_overflow, (64, 68)),
    "ties_one": (lambda: g_ties(False), (64, 68)),
    "ties_two": (lambda: g_ties(True), (64, 68)),
}
CASES = [(name, ef) for name, (_, efs) in GRAPHS.items() for ef in efs]


def handmade(name):
    """(oracle, rows, levels, queries, graph) -- queries[0] is q*"""
    key = ("handmade", name)
    if key not in _CACHE:
        from oracle import oracle_py as O
        g = GRAPHS[name][0]()
        rows = np.zeros((N, D), dtype=np.float32)
        rows[:, 0] = g.r
        lv = np.zeros(N, dtype=np.uint8)
        orc = O.OracleHNSW(M, 32, D, O.VEC_F32)
        orc.import_points(rows, lv)
        nodes = np.arange(N, dtype=np.uint32)
        offs = np.zeros(N + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(g.adj[i]) for i in range(N)])
        flat = np.array([x for i in range(N) for x in g.adj[i]], dtype=np.uint32)
        orc.import_layer(0, nodes, offs, flat)
        orc.set_ep(g.ep)
        noise = np.random.default_rng(7).standard_normal((3, D)).astype(np.float32)
        qs = np.concatenate([np.zeros((1, D), np.float32), noise * np.float32([[2.0 ** -10], [2.0 ** -3], [4.0]])])
        _CACHE[key] = (orc, rows, lv, qs.astype(np.float32), g)
    return _CACHE[key]


def misses(passes):
    """[(pass, the pass after it)] for the ordinary passes that missed"""
    return [(r, passes[i + 1]) for i, r in enumerate(passes[:-1]) if r["ordinary"] and not r["hit"]]


def kept(r, nx):
    """the miss keeps its runner-up: one key below it, and the next pass's runner-up is the same id"""
    return len(r["below"]) == 1 and not r["p_left"] and nx["p"] == r["p"] and nx["c"] == r["below"][0][1]


def assert_pattern(name, ef, g, passes, dist):
    """what the graph's name promises (module docstring), on the replay's passes for q*"""
    ms = misses(passes)
    what = (name, ef, len(passes), len(ms))
    if name in ("one", "stale", "overflow", "ties_one"):
        need = {"one": 40, "stale": 10, "overflow": 12, "ties_one": 20}[name]
        run = best = 0
        for r, nx in ms:
            assert name == "overflow" or len(r["below"]) == 1, (what, r)
            run = run + 1 if kept(r, nx) else 0
            best = max(best, run)
        assert best >= need, (what, best)
    if name in ("two", "five", "ties_two"):
        k = {"two": 2, "five": 5, "ties_two": 2}[name]
        full = [(r, nx) for r, nx in ms if len(r["below"]) == k]
        assert len(full) >= (20 if name == "ties_two" else 40), what
        assert all((nx["c"], nx["p"]) == miss_sim.predicted(r) for r, nx in full), what
    if name in ("ties_one", "ties_two"):
        P = g.info["P"]
        tied = [r for r, _ in ms if all(k[0] == dist[P] for k in r["below"])]
        assert len(tied) >= 20, what
    if name == "stale":
        # the inserts happen while P is being kept: the candidates that make them are expanded between two passes
        # that both have P as their runner-up
        P, chain = g.info["P"], g.info["chain"]
        for c in (chain[2], chain[4], chain[6]):
            i = next(i for i, r in enumerate(passes) if r["c"] == c)
            assert passes[i - 1]["p"] == P and passes[i]["p"] == P and passes[i + 1]["p"] == P and not passes[i]["hit"], what
        assert any(r["hit"] and r["p"] == P for r in passes), what  # ... and P is committed in the end
    if name == "falls":
        left = [(r, nx) for r, nx in ms if r["p_left"]]
        assert len(left) >= 8 and all(len(r["below"]) == 1 and nx["p"] != r["p"] for r, nx in left), (what, len(left))
        if ef == 3:  # kept once, pushed off by the next miss
            again = sum(1 for (r, nx), (r2, _) in zip(ms, ms[1:]) if kept(r, nx) and r2 is nx and r2["p_left"])
            assert again >= 8, (what, again)
    if name == "overflow":
        fat, P2 = g.info["fat"], g.info["P2"]
        assert sum(1 for r, nx in ms if nx["c"] in fat and kept(r, nx)) >= 4, what
        assert sum(1 for r in passes if r["p"] == P2 and not r["ordinary"]) >= 4, what
