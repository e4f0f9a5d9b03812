"""The big merge of the lean kernels' sorted list (search_lean.hip, Lst<R>::merge and LstHT::merge): a
merge of three or more survivors compacts them into LDS, reads them back by broadcast to rank them against the list,
scatters the list and fills the holes.  The fixtures and the CPU replay glue of tests/test_big_merge_host.py (no GPU)
and tests/test_gpu_big_merge.py.

Hand-made layer-0 graphs in the manner of tests/runner_up_miss.py (its Graph class, its one-axis rows: the target query
q* is the origin and row i is (r_i, 0, ..., 0), so that its distance to q* is the integer r_i exactly and equal
distances with different ids are easy to lay).  One layer, N = 8 192 ids of which a few hundred take part.  A merge's
survivors are the wave's keys below the list's last entry once the list is full, every key before; `merges` replays the
two-row pass and records every merge, and what a fixture's name promises is asserted on that record (assert_pattern)
before anything is asked of a GPU:

  s3, s4, s5     every candidate's row holds 3 / 4 / 5 new ids below all before: the smallest big merge, even and odd
  s31, s32       ... 31 / 32 new ids: a full half wave of survivors
  one_entry      the entry point's row holds 20 ids: the list holds one entry when they arrive
  short_of_ef    the same graph: 20 more arrive while the list is short of ef, so that every key survives
  ef3_20         the same graph at ef = 3: 20 survivors into a full list of three
  front          a full list, every survivor in front of its first entry: n_new = ef and m entries are pushed off
  beyond63       64 entries below every survivor: survivors only beyond entry 63, of c's merge and of p's
  across63       survivors on both sides of entries 63 / 64
  tie_survivors  two survivors of one merge at the same distance
  tie_entry      a survivor at the distance of an entry the list holds
  p_big          the committed runner-up's row holds five new ids: a big merge of p's keys (lanes 32 .. 63), after a big
                 merge of c's three
"""
import bisect

import numpy as np

from tests import runner_up_miss as RM

D, M, S0, N, TOPN = RM.D, RM.M, RM.S0, RM.N, RM.TOPN
EFS = (3, 64, 65, 68, 128, 129, 256)  # Lst<1> (3, 64), LstHT (65, 68, 128), Lst<4> (129, 256)

_CACHE = {}


# ---- the replay: tests/tools/miss_sim.replay's pass with every merge recorded ----------------------------------------

def merges(adj0, dist_of, entry, ef, s0=S0):
    """-> (the list, (n_dist, n_exp, sum_deg), merges).  A merge is a dict: kind ('c' | 'p': lanes 0 .. 31 | 32 .. 63),
    n_cur (entries before), fresh (keys that arrived), m (survivors), keys (the survivors, ascending), pos (their
    places in list + survivors sorted, before the cut at ef), before (the list's keys before), n_new."""
    ef = max(1, ef)
    sel, expanded, visited = [entry], set(), {entry[1]}
    counters = [0, 0, 0]
    out = []

    def unexp(k):
        return [e for e in sel if e[1] not in expanded][:k]

    def expand(node):
        expanded.add(node)
        nbrs = [int(x) for x in adj0[node]]
        fresh = list(dict.fromkeys(n for n in nbrs if n not in visited))
        visited.update(fresh)
        counters[0] += len(fresh)
        counters[1] += 1
        counters[2] += len(nbrs)
        if not fresh:
            return []
        return [(float(d), n) for d, n in zip(dist_of(fresh), fresh)]

    def merge(keys, kind):
        full = len(sel) >= ef
        surv = sorted(k for k in keys if not full or k < sel[ef - 1])
        before = list(sel)
        for k in surv:
            bisect.insort(sel, k)
        out.append(dict(kind=kind, n_cur=len(before), fresh=len(keys), m=len(surv), keys=surv,
                        pos=[sel.index(k) for k in surv], before=before, n_new=min(len(sel), ef)))
        del sel[ef:]

    while True:
        u = unexp(2)
        if not u:
            break
        c, p = u[0], (u[1] if len(u) > 1 else None)
        ordinary = p is not None and len(adj0[c[1]]) <= s0 and len(adj0[p[1]]) <= s0
        merge(expand(c[1]), "c")
        if not ordinary:
            continue
        nxt = unexp(1)
        if nxt and nxt[0] == p:
            merge(expand(p[1]), "p")
    return sel, tuple(counters), out


def big(ms, kind=None):
    return [r for r in ms if r["m"] >= 3 and kind in (None, r["kind"])]


# ---- hand-made graphs ------------------------------------------------------------------------------------------------

def g_fan(levels=3, k=20):
    """the entry point's row holds k ids; the smallest of a level holds the next level, every id below all before"""
    g = RM.Graph(31)
    g.ep = x = g.node(3000)
    for j in range(levels):
        level = [g.node(900 - k * j - k + i) for i in range(1, k + 1)]
        for y in level:
            g.edge(x, y)
        x = level[0]
    return g


def g_tail():
    """32 + 32 entries below everything that follows, then rows that land beyond entry 63 and on both sides of it"""
    g = RM.Graph(32)
    g.ep = e = g.node(3000)
    g1 = [g.node(102 + 2 * i) for i in range(32)]
    for y in g1:
        g.edge(e, y)
    for i in range(32):
        g.edge(g1[0], g.node(202 + 2 * i))    # c: entries 32 .. 63
    for i in range(5):
        g.edge(g1[1], g.node(501 + i))        # p, committed: beyond entry 63
    for i in range(4):
        g.edge(g1[2], g.node(401 + i))        # c: beyond entry 63
    for r in (103, 105, 265, 266, 300, 301):
        g.edge(g1[3], g.node(r))              # p, committed: on both sides
    for r in (107, 109, 261, 263):
        g.edge(g1[4], g.node(r))              # c: on both sides
    return g


def g_tied(levels=30):
    """level j: two ids at R_j = 900 - 2 j and one at R_j + 2, the distance of the two of the level before"""
    g = RM.Graph(33)
    P, x = g.start(999, 1000)
    for j in range(1, levels + 1):
        ids = sorted(i for i in g.pool if i not in g.used)[:3]
        a, b, t = g.node(900 - 2 * j, ids[0]), g.node(900 - 2 * j, ids[1]), g.node(902 - 2 * j, ids[2])
        for y in (b, t, a):
            g.edge(x, y)
        x = a  # the smaller id of the two: the next candidate
    return g


def g_pladder(levels=16):
    """pass j: c's row holds three ids just above p (no miss), p's row five ids below everything: p is committed and
    both merges are big"""
    g = RM.Graph(34)
    P, x = g.start(999, 1000)
    c, p, base = x, P, 1000
    for j in range(1, levels + 1):
        for i in (1, 2, 3):
            g.edge(c, g.node(base + i))
        base = 950 - 50 * j
        level = [g.node(base - 10 * i) for i in (4, 3, 2, 1, 0)]  # ascending; level[1] is the next runner-up
        for y in level:
            g.edge(p, y)
        c, p, base = level[0], level[1], base - 30
    return g


# name -> (builder key, builder, the efs at which the pattern is asserted)
GRAPHS = {
    "s3": ("many3", lambda: RM.g_many(3, 30), (64, 68, 129)),
    "s4": ("many4", lambda: RM.g_many(4, 40), (64, 68, 129)),
    "s5": ("many5", lambda: RM.g_many(5, 30), (64, 68, 129)),
    "s31": ("many31", lambda: RM.g_many(31, 5), (64, 68, 129)),
    "s32": ("many32", lambda: RM.g_many(32, 5), (64, 68, 129)),
    "one_entry": ("fan", g_fan, (3, 64, 68, 129)),
    "short_of_ef": ("fan", g_fan, (64, 68, 129)),
    "ef3_20": ("fan", g_fan, (3,)),
    "front": ("many4", lambda: RM.g_many(4, 40), (64, 68, 128)),
    "beyond63": ("tail", g_tail, (65, 68, 128)),
    "across63": ("tail", g_tail, (65, 68, 128)),
    "tie_survivors": ("tied", g_tied, (64, 68, 129)),
    "tie_entry": ("tied", g_tied, (64, 68, 129)),
    "p_big": ("pladder", g_pladder, (64, 68, 129)),
}
PATTERN_CASES = [(name, ef) for name, (_, _, efs) in GRAPHS.items() for ef in efs]
BUILDERS = sorted({key for key, _, _ in GRAPHS.values()})


def graph(key):
    """the graph of a builder key (several names share one)"""
    if ("graph", key) not in _CACHE:
        _CACHE[("graph", key)] = next(b for k, b, _ in GRAPHS.values() if k == key)()
    return _CACHE[("graph", key)]


def handmade(key, dim=D, kind=None):
    """(oracle, rows, levels, queries, graph) of a builder key -- queries[0] is q*, three noisy ones follow"""
    from oracle import oracle_py as O
    kind = O.VEC_F32 if kind is None else kind
    ck = ("handmade", key, dim, kind)
    if ck not in _CACHE:
        g = graph(key)
        rows = np.zeros((N, dim), dtype=np.float32)
        rows[:, 0] = g.r
        lv = np.zeros(N, dtype=np.uint8)
        orc = O.OracleHNSW(M, 32, dim, kind)
        orc.import_points(rows, lv)
        offs = np.zeros(N + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(g.adj[i]) for i in range(N)])
        flat = np.array([x for i in range(N) for x in g.adj[i]], dtype=np.uint32)
        orc.import_layer(0, np.arange(N, dtype=np.uint32), offs, flat)
        orc.set_ep(g.ep)
        noise = np.random.default_rng(7).standard_normal((3, dim)).astype(np.float32)
        qs = np.concatenate([np.zeros((1, dim), np.float32), noise * np.float32([[2.0 ** -10], [2.0 ** -3], [4.0]])])
        _CACHE[ck] = (orc, rows, lv, qs.astype(np.float32), g)
    return _CACHE[ck]


def replayed(key, ef):
    """(list, counters, merges) of q* on a builder key's f32 d = 100 oracle"""
    ck = ("replayed", key, ef)
    if ck not in _CACHE:
        orc, _, _, qs, g = handmade(key)
        dist = orc.distance_batch(qs[0], np.arange(N, dtype=np.uint32))
        assert np.array_equal(dist, g.r)  # distances to q* are the radii, by construction
        adj0 = {i: g.adj[i] for i in range(N)}
        _CACHE[ck] = merges(adj0, lambda ids: dist[ids], RM.entry_of(orc, qs[0]), ef)
    return _CACHE[ck]


def assert_pattern(name, ef, ms):
    """what the fixture's name promises (module docstring), on the replay's merges for q*"""
    bg = big(ms)
    what = (name, ef, len(ms), len(bg))
    if name in ("s3", "s4", "s5", "s31", "s32"):
        k = int(name[1:])
        hit = [r for r in bg if r["m"] == k]
        assert len(hit) >= (20 if k <= 5 else 4), what
        assert any(r["n_cur"] < ef for r in hit) and (ef > 128 or any(r["n_cur"] == ef for r in hit)), what
    if name == "one_entry":
        assert ms[0]["n_cur"] == 1 and ms[0]["m"] == 20 and ms[0]["n_new"] == min(ef, 21), what
    if name == "short_of_ef":
        r = ms[1]
        assert r["n_cur"] == 21 and r["fresh"] == r["m"] == 20 and r["n_new"] == 41 < ef, what
    if name == "ef3_20":
        assert ef == 3 and sum(1 for r in bg if r["n_cur"] == 3 and r["m"] == 20 and r["n_new"] == 3) >= 2, what
    if name == "front":
        hit = [r for r in bg if r["n_cur"] == ef and r["m"] == 4 and r["pos"] == [0, 1, 2, 3] and r["n_new"] == ef]
        assert len(hit) >= 5, what
    if name == "beyond63":
        for kind in ("c", "p"):
            assert any(min(r["pos"]) >= 64 for r in big(ms, kind)), (what, kind)
    if name == "across63":
        for kind in ("c", "p"):
            assert any(min(r["pos"]) < 63 and max(r["pos"]) > 64 for r in big(ms, kind)), (what, kind)
    if name == "tie_survivors":
        assert sum(1 for r in bg if len({k[0] for k in r["keys"]}) < r["m"]) >= 10, what
    if name == "tie_entry":
        assert sum(1 for r in bg if {k[0] for k in r["keys"]} & {k[0] for k in r["before"]}) >= 10, what
    if name == "p_big":
        assert sum(1 for r in big(ms, "p") if r["m"] == 5) >= 10, what
        assert sum(1 for r in big(ms, "c") if r["m"] == 3) >= 10, what
        assert any(r["n_cur"] == ef for r in big(ms, "p")) or ef > 128, what


# ---- the rank / scatter merge restated in numpy (what the kernel's big merge computes, step by step) ------------------

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)


def layout(R, head_tail):
    """entry index of (lane, register): interleaved (entry i = register i % R of lane i / R) or head + tail"""
    lane, r = np.meshgrid(np.arange(64), np.arange(R), indexing="ij")
    return (64 * r + lane) if head_tail else (R * lane + r)


def rank_scatter_merge(lst, n_cur, keys, ef, R, head_tail=False):
    """lst: 64 R u64 keys by entry (ascending, INVALID behind n_cur); keys: the wave's 64 u64 keys (INVALID = none).
    -> (list by entry, n_new), by the kernel's steps: the survivors compacted in lane order (a pad behind them), every
    entry's shift and every survivor's rank counted over the compacted keys two per trip, the entries scattered to
    index + shift, the holes filled with the survivors in rank order."""
    idx = layout(R, head_tail)              # [lane, r] -> entry
    L = lst[idx]                            # the registers
    last = lst[ef - 1] if n_cur >= ef else INVALID
    surv = keys < last
    m = int(surv.sum())
    assert m >= 3
    stage = np.full(66, INVALID, dtype=np.uint64)
    stage[np.cumsum(surv)[surv] - 1] = keys[surv]        # rank among the set bits of the mask
    stage[m] = INVALID                                   # the pad
    shift = np.zeros(L.shape, dtype=np.int64)
    srank = np.zeros(64, dtype=np.int64)
    for t in range((m + 1) // 2):
        for e in stage[2 * t:2 * t + 2]:
            shift += e < L
            srank += e < keys
    n_new = min(n_cur + m, ef)
    perm = np.full(64 * R, INVALID, dtype=np.uint64)
    go = (idx < n_cur) & (idx + shift < n_new)
    perm[(idx + shift)[go]] = L[go]
    sv = np.full(64, INVALID, dtype=np.uint64)
    sv[srank[surv]] = keys[surv]
    holes = np.nonzero((perm == INVALID) & (np.arange(64 * R) < n_new))[0]   # in entry order
    perm[holes] = sv[:len(holes)]
    return perm, n_new


def merge_model(lst, n_cur, keys, ef):
    """sorted(list + survivors)[:ef]"""
    last = lst[ef - 1] if n_cur >= ef else INVALID
    allk = np.sort(np.concatenate([lst[:n_cur], keys[keys < last]]))[:ef]
    return allk, len(allk)


def key_u64(k):
    """a replay key (distance, id) as the kernel's (distance bits << 32 | id)"""
    return (np.uint64(np.float32(k[0]).view(np.uint32)) << np.uint64(32)) | np.uint64(k[1])
