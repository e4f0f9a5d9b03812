"""The lean f32 kernels' upper-layer walk with its adjacency rows requested ahead (search_lean.hip, DESIGN.md 4a: the
entry point's top row is requested under its own distance, the row the walk expands next lives in one register that
an improvement and a descent replace, and the row the walk ends on is handed to the first layer-0 pass as a row fetched
ahead): the fixtures and the CPU replay of tests/test_upper_walk_host.py (no GPU) and tests/test_gpu_upper_walk.py.
The cases aim at that register: a row requested for one node and consumed, replaced or dropped later.

Hand-made upper layers.  N = 2 048 rows of H.synth_rows at d = 100, m = 16 (S0 32, S1 16), as f32 or quant8 rows
(fixture(name, kind): the oracle of that kind ranks the ids, so a case holds for the kind it is built for).  Layer 0 is the
circulant graph with the offsets +-{1, 5, 67, 1031} of tests/graph_shapes.py unless a case replaces a row; the upper
layers are directed rows laid by hand.  One target query q* (queries[0]); the ids are ranked by the oracle's own
distance to q*, and a case takes from three pools: `step` (every id strictly nearer than all steps before it),
`filler` (farther than every step: never wins) and `decoy` (nearer than every step: wins wherever it is looked at).
Where the walk leaves a node without going down through it, the node's row one layer down holds the decoy alone: a
walk that kept the row requested for the old node instead of the new one's goes somewhere else and its counters
differ.

  tower             the entry point (level 5) is nearer than every neighbour on every layer: five descents in a row on
                    rows of degree 2 .. 6, each requested ahead, and the first layer-0 pass on the row requested on
                    layer 1
  stairs_tall       exactly one improvement per layer, every winner of level 5: the row below is the new node's
  stairs_exact      ... every winner's level equals the layer it wins on; the layer-1 winner's row below is its
                    layer-0 row of 32 ids
  runs              1, 2 and 7 improvements in a row on layers 3, 2, 1, then the descent
  ties              two fresh neighbours with equal distance bits (duplicate rows), the larger id first in the row: the
                    smaller id wins and the next expansion is its row (the larger's holds the decoy)
  overflow_up_a/_b  a winner whose rows have degree S1 + 1 and S1 + 33, one reached by an improvement and one by the
                    descent (_a: S1 + 1 by the improvement; _b: S1 + 33), the next winner in the overflow part
  overflow_0        the node that ends layer 1 has a layer-0 row of degree S0 + 1
  empty_walk        the winner's row on its layer has degree 0 and the row below it too
  empty_entry       an entry point (level 2) all of whose rows are empty, layer 0's included: one result
  level0_neighbour  the entry point's layer-1 row lists a node of level 0; every query is that node's stored row plus a
                    little noise, so every query walks into it: the reference answers Err("... not in Graph").  The
                    oracle takes this graph; the product's import_layer refuses it (HNSW_ERR_NODE_NOT_IN_GRAPH: a
                    neighbour below the layer), and so does every other way into a product index, so no kernel ever
                    sees it: tests/test_upper_walk_host.py pins the refusal, and the GPU test runs
  level0_entry      instead: two upper layers, the entry point a node of level 0 (the shape of `misplaced` in
                    tests/graph_shapes.py): its upper_base is the empty slot, no row may be requested from it

Replay.  search_layer(layer, q*, [cur], 1) of the oracle, layer by layer from the entry point: the winner of every
layer, the number of improvements on it (expansions - 1: with one slot in `selected` every improving expansion is
followed by exactly one more) and the row taken on the descent are the ones the case promises.

Built index.  20 000 rows, built on the device (tests/test_gpu_upper_walk.py), 256 queries.
"""
import numpy as np

N, D, M, S0, S1 = 2048, 100, 16, 32, 16
OFFSETS = (1, 5, 67, 1031)
EFS = (10, 64, 68)  # one list register twice, head + tail
TOPN = 10
NQ = 8
N_BUILT, NQ_BUILT = 20000, 256
FIRST_STEP, STEP_GAP = 600, 24  # ranks (farthest first) of the steps; the fillers come from below the first

_CACHE = {}


def world():
    """(rows, queries): queries[0] is q*, then three perturbations of it and four unrelated rows"""
    if "world" not in _CACHE:
        import hnsw_rs_amd as H
        rows = H.synth_rows(0, 0x0A1C0001, 0, N, D)
        qs = H.synth_rows(0, 0x0A1C0002, 0, 5, D)
        noise = np.random.default_rng(0xA1C).standard_normal((3, D)).astype(np.float32)
        near = qs[:1] + noise * np.float32([[2.0 ** -20], [2.0 ** -10], [2.0 ** -4]])
        _CACHE["world"] = (rows, np.concatenate([qs[:1], near, qs[1:]]).astype(np.float32))
    return _CACHE["world"]


F32, QUANT8 = 1, 0  # vector kinds (O.VEC_F32 / O.VEC_QUANT8; the import below checks)


def distances(rows, q, kind=F32):
    """the oracle's own distances of this kind of q to every row"""
    from oracle import oracle_py as O
    assert (O.VEC_F32, O.VEC_QUANT8) == (F32, QUANT8)
    pts = O.OracleHNSW(M, 32, D, kind)
    pts.import_points(rows, np.zeros(len(rows), dtype=np.uint8))
    return pts.distance_batch(q, np.arange(len(rows), dtype=np.uint32))


_BUILD_KIND = [F32]


class Case:
    def __init__(self, name):
        kind = _BUILD_KIND[0]  # (set by fixture(): the pools are ranked by this kind's distances)
        rows, qs = world()
        self.name = name
        self.kind = kind
        self.rows = rows.copy()
        self.queries = qs.copy()
        if ("dist", kind) not in _CACHE:
            _CACHE[("dist", kind)] = distances(rows, qs[0], kind)
        self.dist = _CACHE[("dist", kind)].copy()
        self.order = [int(x) for x in np.lexsort((np.arange(N), self.dist))[::-1]]  # farthest first
        self.n_step = self.n_fill = self.n_decoy = 0
        self.levels = np.zeros(N, dtype=np.uint8)
        ids = np.arange(N)
        self.adj0 = {int(i): [int((i + s * o) % N) for o in OFFSETS for s in (1, -1)] for i in ids}
        self.up = {}       # layer -> {node: [neighbours]}
        self.expect = []   # (layer, winner, improvements), top layer first
        self.descent = {}  # layer the walk leaves -> the row it takes one layer down
        self.ep = None
        self.special = set()

    # ---- pools ----
    def _take(self, id, level):
        assert id not in self.special, (self.name, id)
        self.special.add(id)
        self.levels[id] = level
        return id

    def step(self, level):
        id = self.order[FIRST_STEP + STEP_GAP * self.n_step]
        self.n_step += 1
        assert FIRST_STEP + STEP_GAP * self.n_step < N - 64
        return self._take(id, level)

    def filler(self, level):
        id = self.order[self.n_fill]
        self.n_fill += 1
        assert self.n_fill < FIRST_STEP
        return self._take(id, level)

    def fillers(self, k, level):
        return [self.filler(level) for _ in range(k)]

    def decoy(self, level):
        id = self.order[N - 1 - self.n_decoy]
        self.n_decoy += 1
        return self._take(id, level)

    # ---- rows ----
    def row(self, node, layer, nbrs):
        nbrs = [int(x) for x in nbrs]
        assert node not in nbrs and len(set(nbrs)) == len(nbrs), (self.name, node, layer)
        assert self.levels[node] >= layer, (self.name, node, layer)
        if layer == 0:
            self.adj0[node] = nbrs
        else:
            self.up.setdefault(layer, {})[node] = nbrs

    def layers(self):
        """[layer 0's rows, layer 1's, ...]: every node on every layer up to its level, rows empty unless set"""
        top = int(self.levels.max())
        out = [self.adj0]
        for l in range(1, top + 1):
            rows = {int(i): [] for i in np.nonzero(self.levels >= l)[0]}
            rows.update(self.up.get(l, {}))
            out.append(rows)
        return out


def csr(adj):
    nodes = sorted(adj)
    offs = np.zeros(len(nodes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(adj[n]) for n in nodes])
    flat = np.array([x for n in nodes for x in adj[n]], dtype=np.uint32)
    return np.array(nodes, dtype=np.uint32), offs, flat


# ---- the cases -------------------------------------------------------------------------------------------------------

def tower():
    c = Case("tower")
    c.ep = c.step(5)
    for l in range(5, 0, -1):
        c.row(c.ep, l, c.fillers(l + 1, l))
        c.expect.append((l, c.ep, 0))
        if l >= 2:
            c.descent[l] = l  # degrees: the row taken when layer l ends has l neighbours
    c.descent[1] = 8
    return c


def stairs(exact):
    c = Case("stairs_exact" if exact else "stairs_tall")
    dz = c.decoy(5)
    cur = c.ep = c.step(5)
    for l in range(5, 0, -1):
        w = c.step(l if exact else 5)
        c.row(cur, l, [w] + c.fillers(2, l))
        c.row(w, l, [cur] + c.fillers(1, l))
        c.row(cur, l - 1, [dz])  # the old node's row below: not the one the descent takes
        c.expect.append((l, w, 1))
        cur = w
    # the layer-1 winner's layer-0 row: 32 ids, the nearer half behind the farther one
    c.row(cur, 0, c.fillers(16, 0) + [c.step(0) for _ in range(16)])
    c.descent = {5: 3, 4: 3, 3: 3, 2: 3, 1: 32}
    return c


def runs():
    c = Case("runs")
    dz = c.decoy(3)
    cur = c.ep = c.step(3)
    for l, k in ((3, 1), (2, 2), (1, 7)):
        for _ in range(k):
            w = c.step(3)
            c.row(cur, l, [w] + c.fillers(2, l))
            c.row(cur, l - 1, [dz])  # replaced by the winner's at the improvement
            cur = w
        c.row(cur, l, c.fillers(2, l))
        c.expect.append((l, cur, k))
    c.descent = {3: 3, 2: 3, 1: 8}
    return c


def ties():
    c = Case("ties")
    dz = c.decoy(2)
    cur = c.ep = c.step(2)
    for l in (2, 1):
        a, b = c.step(2), c.step(2)
        small, big = min(a, b), max(a, b)
        c.rows[big] = c.rows[small]
        c.dist[big] = c.dist[small]
        x = c.step(2)
        c.row(cur, l, [big, small] + c.fillers(1, l))
        c.row(small, l, [x])
        c.row(big, l, [dz])
        c.row(x, l, c.fillers(1, l))
        c.row(cur, l - 1, [dz])
        c.row(small, l - 1, [dz])
        c.expect.append((l, x, 2))
        cur = x
    c.descent = {2: 3, 1: 8}
    return c


def overflow_up(first, second, name):
    """the winner's layer-2 row (reached by an improvement) has `first` neighbours, its layer-1 row (reached by the
    descent) `second`; layer 1's winner is the last of that row"""
    c = Case(name)
    c.ep = c.step(2)
    h = c.step(2)
    w = c.step(1)
    c.row(c.ep, 2, [h] + c.fillers(1, 2))
    c.row(h, 2, [c.ep] + c.fillers(first - 1, 2))
    c.row(h, 1, c.fillers(second - 1, 1) + [w])
    c.row(w, 1, [h] + c.fillers(1, 1))
    c.expect = [(2, h, 1), (1, w, 1)]
    c.descent = {2: second, 1: 8}
    c.degrees = {(h, 2): first, (h, 1): second}
    return c


def overflow_0():
    c = Case("overflow_0")
    c.ep = c.step(1)
    w = c.step(1)
    c.row(c.ep, 1, [w] + c.fillers(1, 1))
    c.row(w, 1, [c.ep])
    c.row(w, 0, c.adj0[w] + c.fillers(S0 + 1 - len(c.adj0[w]), 0))
    c.expect = [(1, w, 1)]
    c.descent = {1: S0 + 1}
    return c


def empty_walk():
    c = Case("empty_walk")
    dz = c.decoy(3)
    c.ep = c.step(3)
    w = c.step(3)
    v = c.step(1)
    c.row(c.ep, 3, [w])
    c.row(c.ep, 2, [dz])
    c.row(w, 3, [])
    c.row(w, 2, [])
    c.row(w, 1, [v] + c.fillers(1, 1))
    c.row(v, 1, [])
    c.expect = [(3, w, 1), (2, w, 0), (1, v, 1)]
    c.descent = {3: 0, 2: 2, 1: 8}
    return c


def empty_entry():
    c = Case("empty_entry")
    c.ep = c.step(2)
    c.row(c.ep, 0, [])
    c.expect = [(2, c.ep, 0), (1, c.ep, 0)]
    c.descent = {2: 0, 1: 0}
    return c


def level0_neighbour():
    c = Case("level0_neighbour")
    c.ep = c.step(1)
    z = c.decoy(0)
    c.row(c.ep, 1, c.fillers(2, 1) + [z])
    noise = np.random.default_rng(0xA1C0).standard_normal((NQ, D)).astype(np.float32)
    c.queries = (c.rows[z][None, :] + noise * np.float32(2.0 ** -8)).astype(np.float32)
    c.queries[0] = c.rows[z]
    c.z = z
    return c


def level0_entry():
    """what the product's import lets through of it: the entry point itself is the node of level 0"""
    c = Case("level0_entry")
    top = c.step(2)
    c.row(top, 2, c.fillers(2, 2))
    c.row(top, 1, c.fillers(2, 1))
    c.ep = c.step(0)
    return c


CASES = {
    "tower": tower,
    "stairs_tall": lambda: stairs(False),
    "stairs_exact": lambda: stairs(True),
    "runs": runs,
    "ties": ties,
    "overflow_up_a": lambda: overflow_up(S1 + 1, S1 + 33, "overflow_up_a"),
    "overflow_up_b": lambda: overflow_up(S1 + 33, S1 + 1, "overflow_up_b"),
    "overflow_0": overflow_0,
    "empty_walk": empty_walk,
    "empty_entry": empty_entry,
}
REFUSED = {"level0_neighbour": level0_neighbour, "level0_entry": level0_entry}  # the reference answers an error


def fixture(name, kind=F32):
    """(case, oracle of this vector kind holding its points and graph)"""
    if (name, kind) not in _CACHE:
        from oracle import oracle_py as O
        _BUILD_KIND[0] = kind
        try:
            c = {**CASES, **REFUSED}[name]()
        finally:
            _BUILD_KIND[0] = F32
        orc = O.OracleHNSW(M, 32, D, kind)
        orc.import_points(c.rows, c.levels)
        for l, adj in enumerate(c.layers()):
            orc.import_layer(l, *csr(adj))
        orc.set_ep(c.ep)
        _CACHE[(name, kind)] = (c, orc)
    return _CACHE[(name, kind)]


def product(name, kind=F32):
    """the product index of a fixture (imported, nothing is built)"""
    key = ("product", name, kind)
    if key not in _CACHE:
        import hnsw_rs_amd as H
        c, _ = fixture(name, kind)
        idx = H.HNSW.new(M, 32, D, kind)
        idx.import_points(c.rows, c.levels)
        for l, adj in enumerate(c.layers()):
            idx.import_layer(l, *csr(adj))
        idx.set_ep(c.ep)
        _CACHE[key] = idx
    return _CACHE[key]


# ---- the replay ------------------------------------------------------------------------------------------------------

def replay(orc, q):
    """the greedy walk down the upper layers -> [(layer, winner, improvements, degree of the row taken on the descent)]"""
    out, cur = [], orc.ep
    for l in range(orc.nb_layers - 1, 0, -1):
        ids, _, stats = orc.search_layer(l, q, [cur], 1)
        cur = int(ids[0])
        out.append((l, cur, int(stats[1]) - 1, len(orc.neighbors(l - 1, cur))))
    return out


def assert_pattern(name, kind=F32):
    """what the case's name promises (module docstring), on the replay for q*"""
    c, orc = fixture(name, kind)
    got = replay(orc, c.queries[0])
    assert [g[:3] for g in got] == c.expect, (name, got, c.expect)
    assert {g[0]: g[3] for g in got} == c.descent, (name, got, c.descent)
    d = orc.distance_batch(c.queries[0], np.arange(N, dtype=np.uint32))
    if name == "ties":
        for l in (2, 1):
            big, small = c.up[l][_start(c, got, l)][:2]
            winner = [g[1] for g in got if g[0] == l][0]
            assert big > small and d[big:big + 1].view(np.uint32)[0] == d[small:small + 1].view(np.uint32)[0], (name, l)
            assert c.up[l][small] == [winner] and c.up[l][big] != c.up[l][small], (name, l)
    if name.startswith("overflow_up"):
        for (node, l), deg in c.degrees.items():
            assert len(orc.neighbors(l, node)) == deg and deg > S1, (name, node, l)
        assert sorted(c.degrees.values()) == [S1 + 1, S1 + 33], name
    if name == "stairs_exact":
        assert all(c.levels[w] == l for l, w, _, _ in got), (name, got)
    if name == "empty_entry":
        ids, _, counts, _ = orc.search_batch(c.queries, TOPN, 64)
        assert (counts == 1).all() and (ids[:, 0] == c.ep).all(), (name, counts)
    return got


def _start(c, got, layer):
    """the node layer `layer` starts from: the entry point on the top layer, else the winner of the layer above"""
    above = [g for g in got if g[0] == layer + 1]
    return above[0][1] if above else c.ep


def assert_refused(name, kind=F32):
    """every query of the case walks into the node of level 0: the oracle raises for each of them alone"""
    from oracle import oracle_py as O
    c, orc = fixture(name, kind)
    assert orc.nb_layers > 1, name
    if name == "level0_entry":
        assert c.levels[c.ep] == 0, name
    else:
        assert c.levels[c.z] == 0 and c.z in c.up[1][c.ep], name
    for q in c.queries:
        if name == "level0_neighbour":
            d = orc.distance_batch(q, np.array([c.z, c.ep] + [x for x in c.up[1][c.ep] if x != c.z], dtype=np.uint32))
            assert (d[0] < d[1:]).all(), (name, d)
        try:
            orc.search_batch(q[None, :], TOPN, 64)
        except O.OracleError as e:
            assert e.code == -3, (name, e)
        else:
            raise AssertionError("%s: the oracle answers" % name)
