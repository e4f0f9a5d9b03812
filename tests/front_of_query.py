"""The front of a query in the lean f32 kernels (search_lean.hip, DESIGN.md 4a and 10, "The front of the query"):
query staging, the entry point, the first expansion of the upper-layer walk, the walk's visited filter with its claims
made while the rows are in flight, and the transition to the layer-0 table.  The fixtures and the CPU replay of
tests/test_front_of_query_host.py (no GPU) and tests/test_gpu_front_of_query.py, in the style of tests/upper_walk.py,
whose world (2 048 rows at d = 100, m = 16: S0 32, S1 16), pools and Case they use.

Hand-laid upper layers; layer 0 is upper_walk's circulant graph unless a case replaces a row.

  deg1 / deg2 / deg16   two layers; the entry point's top row has degree 1, 2, S1: the winner first, fillers behind it
  empty_top             two layers, the entry point's top row is empty
  one_layer             every node of level 0: no upper layer, the entry point goes straight to layer 0
  three_layers          the entry point of level 2, one improvement per layer
  dup_small / dup_large a neighbour in the top row whose stored row is the entry point's (equal distance bits): with the
                        smaller id it wins and the walk goes on from it, with the larger id it does not
  top_overflow          a top row of degree S1 + 1: its last id sits in the overflow part, and wins
  nan_entry             the entry point's distance is a NaN: the reference panics at its first comparison.  A product
                        index cannot hold a NaN in a stored row (import_points refuses it, tests/test_front_of_query_host.py
                        pins that), so the stored row holds + infinity in one element, which the import takes, and so does
                        every query of the case: inf - inf in that element
  nan_neighbour         the same in the stored row of a top-row neighbour: the entry point's distance is + infinity, the
                        neighbour's a NaN, and the reference panics at the first expansion
  bucket                ids chosen by the home bucket of the upper layers' visited table (home(), below): the entry
                        point's top row holds five ids of one home bucket -- they race for its four slots, and one ends
                        in the next bucket, which one the hardware decides -- and a sixth id of another bucket, the
                        nearest, which wins.  The winner's row lists all five again, so whichever of them sits in the
                        next bucket meets a full home bucket at its look: its row is requested, its claim finds it
                        present, and its distance must not count (n_dist would be one too many; it cannot change an
                        id: a revisited id is never nearer than the best of the ids visited)
  quarters              the first layer-0 pass expands a row of 32 ids, eight in each quarter of the layer-0 table: the
                        whole table is emptied at the transition today, and a clear split over the kernel (built once
                        and taken out) has to leave every quarter empty as well

Where the reference answers, the oracle is the expectation; where it panics (nan_*), EXPECT_NAN states the counters the
reference had reached: the status for every query, count 0, ids all ones.
"""
import numpy as np

from tests import upper_walk as UW

N, D, M, S0, S1, TOPN = UW.N, UW.D, UW.M, UW.S0, UW.S1, UW.TOPN
EFS = UW.EFS  # 10 and 64: one list register; 68: head + tail
SLOTS_LOG2 = 12  # the visited table of these ef (default_slots_log2): 4 096 slots on layer 0, a quarter on the upper layers

_CACHE = {}


def home(ids, slots_log2):
    """Visited::home: the home bucket (four slots) of an id in a table of 1 << slots_log2 slots"""
    x = (np.asarray(ids, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(32 - (slots_log2 - 2))).astype(np.int64)


def home_upper(ids):
    return home(ids, SLOTS_LOG2 - 2)


def quarter_layer0(ids):
    return home(ids, SLOTS_LOG2) >> (SLOTS_LOG2 - 2 - 2)


def _top_degree(k):
    c = UW.Case("deg%d" % k)
    c.ep = c.step(1)
    w = c.step(1)
    c.row(c.ep, 1, [w] + c.fillers(k - 1, 1))
    c.row(w, 1, [c.ep])
    c.top_degree = k
    c.winner = w
    return c


def empty_top():
    c = UW.Case("empty_top")
    c.ep = c.step(1)
    c.top_degree = 0
    c.winner = c.ep
    return c


def one_layer():
    c = UW.Case("one_layer")
    c.ep = c.step(0)
    c.winner = c.ep
    return c


def three_layers():
    c = UW.Case("three_layers")
    cur = c.ep = c.step(2)
    for l in (2, 1):
        w = c.step(2)
        c.row(cur, l, [w] + c.fillers(2, l))
        c.row(w, l, [cur])
        cur = w
    c.top_degree = 3
    c.winner = cur
    return c


def _dup(small_wins):
    c = UW.Case("dup_small" if small_wins else "dup_large")
    a, b = c.step(1), c.step(1)
    c.ep, nbr = (max(a, b), min(a, b)) if small_wins else (min(a, b), max(a, b))
    c.rows[nbr] = c.rows[c.ep]
    x = c.step(1)  # nearer than both: reached only through the neighbour's row
    c.row(c.ep, 1, c.fillers(1, 1) + [nbr] + c.fillers(1, 1))
    c.row(nbr, 1, [x])
    c.row(x, 1, c.fillers(1, 1))
    c.top_degree = 3
    c.nbr = nbr
    c.winner = x if small_wins else c.ep
    return c


def top_overflow():
    c = UW.Case("top_overflow")
    c.ep = c.step(1)
    w = c.step(1)
    c.row(c.ep, 1, c.fillers(S1, 1) + [w])
    c.row(w, 1, [c.ep])
    c.top_degree = S1 + 1
    c.winner = w
    return c


def _nan(in_entry):
    c = UW.Case("nan_entry" if in_entry else "nan_neighbour")
    c.ep = c.step(1)
    w = c.step(1)
    f = c.fillers(1, 1)
    c.row(c.ep, 1, [w] + f)
    c.row(w, 1, [c.ep])
    c.nan_row = c.ep if in_entry else f[0]
    c.rows[c.nan_row, 7] = np.inf
    c.queries[:, 7] = np.inf
    c.top_degree = 2
    return c


def bucket():
    c = UW.Case("bucket")
    rank = {id: r for r, id in enumerate(c.order)}  # farthest first
    hb = home_upper(np.arange(N))
    # a home bucket of the upper table with five ids or more
    nbuckets = 1 << (SLOTS_LOG2 - 4)
    b = int(np.argmax(np.bincount(hb, minlength=nbuckets)))
    five = sorted((int(i) for i in np.nonzero(hb == b)[0]), key=lambda i: rank[i])[:5]
    assert len(five) == 5
    for i in five:
        c._take(i, 1)
    # of other home buckets, and not of the next one, which holds the id that loses the race and nothing else: the
    # winner (nearer than all five), the entry point (farther than the winner), the one fresh id of the winner's row
    others = [i for i in c.order if hb[i] not in (b, (b + 1) % nbuckets)]
    near = [i for i in others if rank[i] > max(rank[x] for x in five)]
    w = c._take(near[-1], 1)
    c.ep = c._take(near[0], 1)
    far = c._take(others[0], 1)
    c.row(c.ep, 1, five[:2] + [w] + five[2:])
    c.row(w, 1, five + [far])
    c.five, c.home_bucket, c.winner, c.top_degree = five, b, w, 6
    return c


def quarters():
    c = UW.Case("quarters")
    c.ep = c.step(1)
    c.row(c.ep, 1, c.fillers(1, 1))
    qt = quarter_layer0(np.arange(N))
    row = []
    for k in range(4):
        row += [int(i) for i in np.nonzero(qt == k)[0] if int(i) not in c.special][:8]
    c.row(c.ep, 0, row)
    c.top_degree = 1
    c.winner = c.ep
    c.row0 = row
    return c


CASES = {
    "deg1": lambda: _top_degree(1),
    "deg2": lambda: _top_degree(2),
    "deg16": lambda: _top_degree(S1),
    "empty_top": empty_top,
    "one_layer": one_layer,
    "three_layers": three_layers,
    "dup_small": lambda: _dup(True),
    "dup_large": lambda: _dup(False),
    "top_overflow": top_overflow,
    "bucket": bucket,
    "quarters": quarters,
}
NAN_CASES = {"nan_entry": lambda: _nan(True), "nan_neighbour": lambda: _nan(False)}
# (n_dist, n_exp, sum_deg) the reference had reached when it panicked: the entry point's distance alone; the entry
# point's and the two fresh neighbours' of the first expansion
EXPECT_NAN = {"nan_entry": (1, 0, 0), "nan_neighbour": (3, 1, 2)}


def fixture(name):
    """(case, f32 oracle holding its points and graph)"""
    if name not in _CACHE:
        from oracle import oracle_py as O
        c = {**CASES, **NAN_CASES}[name]()
        orc = O.OracleHNSW(M, 32, D, UW.F32)
        orc.import_points(c.rows, c.levels)
        for l, adj in enumerate(c.layers()):
            orc.import_layer(l, *UW.csr(adj))
        orc.set_ep(c.ep)
        _CACHE[name] = (c, orc)
    return _CACHE[name]


def product(name):
    key = ("product", name)
    if key not in _CACHE:
        import hnsw_rs_amd as H
        c, _ = fixture(name)
        idx = H.HNSW.new(M, 32, D, UW.F32)
        idx.import_points(c.rows, c.levels)
        for l, adj in enumerate(c.layers()):
            idx.import_layer(l, *UW.csr(adj))
        idx.set_ep(c.ep)
        _CACHE[key] = idx
    return _CACHE[key]


def expected(name, ef):
    """the oracle's answer for the case's queries, computed once per (case, ef) and shared"""
    key = ("expected", name, ef)
    if key not in _CACHE:
        c, orc = fixture(name)
        _CACHE[key] = orc.search_batch(c.queries, TOPN, ef, nthreads=8)
    return _CACHE[key]


def assert_pattern(name):
    """what the case's name promises, on the oracle's search_layer for q*"""
    c, orc = fixture(name)
    q = c.queries[0]
    top = orc.nb_layers - 1
    assert orc.nb_layers == {"one_layer": 1, "three_layers": 3}.get(name, 2), name
    if name == "one_layer":
        assert int(c.levels.max()) == 0
        return
    assert len(orc.neighbors(top, c.ep)) == c.top_degree, name
    got = UW.replay(orc, q)
    assert got[-1][1] == c.winner, (name, got, c.winner)
    ids, _, stats = orc.search_layer(top, q, [c.ep], 1)
    if name.startswith("dup"):
        d = orc.distance_batch(q, np.array([c.ep, c.nbr], dtype=np.uint32)).view(np.uint32)
        assert d[0] == d[1] and (c.nbr < c.ep) == (name == "dup_small"), name
        assert int(stats[1]) == (3 if name == "dup_small" else 1), (name, stats)  # expansions on the top layer
    if name == "top_overflow":
        assert c.top_degree > S1 and c.up[top][c.ep][-1] == c.winner, name
    if name == "bucket":
        hb = home_upper(c.five)
        assert (hb == c.home_bucket).all() and len(set(c.five)) == 5, name
        assert home_upper([c.ep])[0] not in (c.home_bucket, (c.home_bucket + 1) % (1 << (SLOTS_LOG2 - 4))), name
        assert home_upper([c.winner])[0] not in (c.home_bucket, (c.home_bucket + 1) % (1 << (SLOTS_LOG2 - 4))), name
        # whichever of the five lost the race for the four slots, the winner's row lists it again
        assert set(c.five) < set(c.up[1][c.winner]) and set(c.five) < set(c.up[1][c.ep]), name
        # two expansions; the second meets five visited ids and one fresh one
        assert int(stats[1]) == 2 and int(stats[0]) == 1 + 6 + 1 and int(stats[2]) == 12, (name, stats)
    if name == "quarters":
        assert sorted(np.bincount(quarter_layer0(c.row0), minlength=4)) == [8, 8, 8, 8], name
        assert sorted(int(x) for x in orc.neighbors(0, c.winner)) == sorted(c.row0), name


def assert_panics(name):
    from oracle import oracle_py as O
    c, orc = fixture(name)
    assert not np.isnan(c.rows).any() and np.isinf(c.rows).sum() == 1 and np.isinf(c.queries[:, 7]).all(), name
    d = orc.distance_batch(c.queries[0], np.array([c.nan_row, c.ep, c.up[1][c.ep][0]], dtype=np.uint32))
    assert np.isnan(d[0]) and (name == "nan_entry" or (np.isinf(d[1]) and not np.isnan(d[2]))), (name, d)
    for q in c.queries:
        try:
            orc.search_batch(q[None, :], TOPN, 64)
        except O.OracleError as e:
            assert e.code == -2, (name, e)
        else:
            raise AssertionError("%s: the oracle answers" % name)
