"""One merge per committed pass in the lean f32 kernels (search_lean.hip): a pass whose runner-up p is
committed -- no fresh key of its candidate c sorts below p, known from the pass's own keys -- claims p's slots first and
merges the keys of both rows once.  The fixtures and the CPU replay glue of tests/test_one_merge_commit_host.py (no GPU)
and tests/test_gpu_one_merge_commit.py.

Hand-made layer-0 graphs in the manner of tests/frontier.py (its Script: one-axis rows, the distance of row i to the
target query q* is the integer r_i exactly; a row is given to a pass's c or to its committed p).  The replay here runs
every committed pass both ways -- c's keys merged, then p's; and both rows' keys in one merge against the bound as it
stood before the pass -- and asserts the same list.  What a row's name promises is asserted on the replay's passes
(`states`) before anything is asked of a GPU.  With (x, y) the keys of c's and of p's row below the bound before the merge:

  sv_x_y            x and y of 0, 1, 2, 3 (more than the shift path takes) and 16: (0,0) (1,0) (0,1) (1,1) (2,1) (2,2)
                    (3,0) (0,3) (16,16)
  p_front           a key of p in front of every key of c
  tie_c_small, tie_p_small   a key of c and a key of p at one distance, the smaller id on either side
  c_pushes_p        a key of p below the bound before the pass that c's survivor keeps out of the list
  p_pushes_c        a survivor of c that p's survivor pushes off the end
  p_pa, p_ab, p_at_b   a survivor of p between p and a, between a and b, and at b's distance
  shared            a neighbour of p that c inserted in the same pass
  taken             a neighbour of p whose slot c took for another id of the same home bucket in the same pass
  full              a neighbour of p whose home bucket was full before the pass
  race              two neighbours of p of one home bucket, both fresh: two lanes claim one slot
  miss_then_fold, fold_then_miss   a miss directly before and directly after a committed pass
  kept_fold         a runner-up kept over a miss (one key below it) and committed by the pass after, with survivors
  commit40          p committed 40 times in a row
`small` lays committed passes for ef 2 .. 4 whose rows hold more keys than the list (at ef 1 there is no runner-up);
tests/runner_up_miss.py's `overflow` gives rows with an overflow pointer on c and on p.  Three more graphs of three
passes each (at the end of the file): `full_rows` (one merge of 64 survivors), `visited` (the table's limit reached by
p's claims, by c's, and just missed) and `nan_case` (a NaN distance of a neighbour of c, of p, of both: import_points
refuses a NaN in a row, so the row holds +inf in a component where the query holds +inf too).
"""
import bisect

import numpy as np

from tests import frontier as FR
from tests import runner_up_miss as RM

D, M, S0, N, TOPN = FR.D, FR.M, FR.S0, FR.N, FR.TOPN
EFS_WIDE = FR.EFS_WIDE
EFS_SMALL = FR.EFS_SMALL
EFS = EFS_SMALL + EFS_WIDE
INF = (float("inf"), 1 << 62)  # no bound: above every key, the ones at distance +inf included

_CACHE = {}


# ---- the replay: every committed pass merged both ways ----------------------------------------------------------------

def replay(adj0, dist_of, entry, ef, s0=S0):
    """-> (list, (n_dist, n_exp, sum_deg), passes, status).  status is "ok" or "nan": a NaN distance among the fresh
    neighbours of an expansion ends the walk behind that expansion's counters (the list is void then).  A pass is a
    dict: c, p, F (the first four unexpanded keys at the pick), fold (p committed), miss (an ordinary pass that did not
    commit); of a fold: kc / kp (the fresh keys of c's and of p's row), last (the bound before the pass), in_c / in_p
    (those of them in the list afterwards), dup (neighbours of p that c's row inserted in this pass); of every pass: ids
    (the ids it inserted into the visited set)."""
    ef = max(1, ef)
    sel, expanded, visited = [entry], set(), {entry[1]}
    counters = [0, 0, 0]

    def expand(node):
        expanded.add(node)
        nbrs = [int(x) for x in adj0[node]]
        fresh = list(dict.fromkeys(n for n in nbrs if n not in visited))
        visited.update(fresh)
        counters[0] += len(fresh)
        counters[1] += 1
        counters[2] += len(nbrs)
        return [(float(d), n) for d, n in zip(dist_of(fresh), fresh)] if fresh else []

    def merged(lst, keys):
        last = lst[ef - 1] if len(lst) >= ef else INF
        out = list(lst)
        for k in keys:
            if k < last:
                bisect.insort(out, k)
        return out[:ef]

    nan = lambda keys: any(k[0] != k[0] for k in keys)
    passes = []
    while True:
        u = [e for e in sel if e[1] not in expanded]
        if not u:
            break
        F = u[:4]
        c, p = F[0], (F[1] if len(F) > 1 else None)
        ordinary = p is not None and len(adj0[c[1]]) <= s0 and len(adj0[p[1]]) <= s0
        rec = dict(c=c[1], p=None if p is None else p[1], F=F, fold=False, miss=False)
        passes.append(rec)
        kc = expand(c[1])
        rec["ids"] = {k[1] for k in kc}
        if nan(kc):
            return sel, tuple(counters), passes, "nan"
        if not ordinary or any(k < p for k in kc):
            rec["miss"] = ordinary
            sel = merged(sel, kc)
            continue
        fresh_c = {k[1] for k in kc}
        dup = [n for n in adj0[p[1]] if n in fresh_c]
        kp = expand(p[1])
        rec["ids"] |= {k[1] for k in kp}
        if nan(kp):
            return sel, tuple(counters), passes, "nan"
        last = sel[ef - 1] if len(sel) >= ef else INF
        two = merged(merged(sel, kc), kp)
        sel = merged(sel, kc + kp)
        assert sel == two, (ef, rec)
        rec.update(fold=True, kc=kc, kp=kp, last=last, dup=dup, in_c=[k for k in kc if k in sel], in_p=[k for k in kp if k in sel])
    return sel, tuple(counters), passes, "ok"


def states(passes, g=None):
    """the names of the module docstring that the passes of one walk show"""
    out = set()
    run = 0
    size = lambda n: "16" if n >= 16 else str(min(n, 3))
    hb = lambda i: int(RM.GS.home_bucket([i], 12)[0])
    seen = set()  # ids inserted before the pass
    for i, r in enumerate(passes):
        run = run + 1 if r["fold"] else 0
        if run >= 40:
            out.add("commit40")
        if r["fold"]:
            kc, kp, last, F = r["kc"], r["kp"], r["last"], r["F"]
            bc, bp = [k for k in kc if k < last], [k for k in kp if k < last]
            out.add("sv_%s_%s" % (size(len(bc)), size(len(bp))))
            if bc and bp and min(bp) < min(bc):
                out.add("p_front")
            for x in bc:
                for y in bp:
                    if x[0] == y[0]:
                        out.add("tie_c_small" if x[1] < y[1] else "tie_p_small")
            if r["in_c"] and any(k not in r["in_p"] for k in bp) and max(r["in_c"]) < min(k for k in bp if k not in r["in_p"]):
                out.add("c_pushes_p")
            if r["in_p"] and any(k not in r["in_c"] and k < last for k in kc):
                out.add("p_pushes_c")
            if len(F) == 4:
                out |= {"p_pa"} if any(F[1] < k < F[2] for k in r["in_p"]) else set()
                out |= {"p_ab"} if any(F[2] < k < F[3] for k in r["in_p"]) else set()
                out |= {"p_at_b"} if any(k[0] == F[3][0] for k in r["in_p"]) else set()
            if len(bc) + len(bp) > len(r["in_c"]) + len(r["in_p"]):
                out.add("cut")
            if r["dup"]:
                out.add("shared")
            if g is not None:
                ids_c, ids_p = [k[1] for k in kc], [k[1] for k in kp]
                if any(hb(y) == hb(z) for y in ids_p for z in ids_c):
                    out.add("taken")
                if any(sum(1 for z in seen if hb(z) == hb(y)) >= 4 for y in ids_p):
                    out.add("full")
                if len({hb(y) for y in ids_p}) < len(ids_p):
                    out.add("race")
            if i > 0 and passes[i - 1]["miss"]:
                out.add("miss_then_fold")
                if passes[i - 1]["p"] == r["p"] and bp:
                    out.add("kept_fold")
            if i + 1 < len(passes) and passes[i + 1]["miss"]:
                out.add("fold_then_miss")
        seen |= r["ids"]
    return out


# ---- the scripts ------------------------------------------------------------------------------------------------------

def gaps(s, start, n):
    """n unused integer radii, one in each of n gaps of the model's list from entry `start` on"""
    out, i = [], s.cur.index(start)
    while len(out) < n:
        assert i + 1 < len(s.cur), (s.ef, n)
        lo, hi = int(s.cur[i][0]), int(s.cur[i + 1][0])
        if hi - lo >= 2:
            out.append(((lo + hi) // 2, None))  # (the middle: both halves keep room for later rows)
        i += 1
    return out


def free_ids(s, n):
    ids = [i for i in range(100, N) if i not in s.g.used][:n]
    return ids


def wide(ef):
    """the script for a list of at least 64 entries"""
    if ("wide", ef) in _CACHE:
        return _CACHE[("wide", ef)]
    s = FR.Script(ef)
    s.row("one_entry", [s.next_lattice()])
    s.fill(ef)
    assert len(s.cur) == ef and len(s.unexp()) >= 40
    hold = {}

    def pair(name, c_nodes, p_nodes):
        """c's row from c_nodes(F), then -- it puts nothing below p -- p's row from p_nodes(F of that pass)"""
        def first(F):
            hold["F"] = F
            return c_nodes(F)
        s.c_row(name + "_c", first)
        s.p_row(name + "_p", p_nodes(hold["F"]))

    # (sixteen and sixteen first: while b is near the front there are sixteen gaps behind it)
    for x, y in ((16, 16),):
        pair("sv_%d_%d" % (x, y), lambda F, x=x: gaps(s, F[3], x), lambda F, y=y: gaps(s, F[3], y))
    # the last gap: a < b, both below the bound
    def last_two(F):
        b, a = s.below(ef - 1, 2)
        hold["a"], hold["b"] = a, b
        return [a]
    pair("c_pushes_p", last_two, lambda F: [hold["b"]])
    def last_two_rev(F):
        b, a = s.below(ef - 1, 2)
        hold["a"], hold["b"] = a, b
        return [b]
    pair("p_pushes_c", last_two_rev, lambda F: [hold["a"]])
    pair("p_pa", lambda F: [], lambda F: [s.between(F[1], F[2])])
    pair("p_ab", lambda F: [], lambda F: [s.between(F[2], F[3])])
    pair("p_at_b", lambda F: [], lambda F: [(F[3][0], free_ids(s, 1)[0])])
    # a committed pass, a miss with one key below its runner-up, and the kept runner-up committed with survivors
    pair("before_miss", lambda F: gaps(s, F[3], 1), lambda F: [])
    s.c_row("miss", lambda F: [s.between(F[0], F[1])])
    pair("kept", lambda F: [], lambda F: gaps(s, F[3], 2))
    pair("p_front", lambda F: gaps(s, F[3], 2), lambda F: s.front(1))
    for c_small in (True, False):
        def tie_c(F):
            hold["r"] = gaps(s, F[3], 1)[0][0]
            lo, hi = free_ids(s, 2)
            hold["ids"] = (lo, hi) if c_small else (hi, lo)
            return [(hold["r"], hold["ids"][0])]
        pair("tie", tie_c, lambda F: [(hold["r"], hold["ids"][1])])
    # a neighbour of p that c inserted in this pass: the edge goes in behind the model's back (the id adds no key)
    pair("shared", lambda F: gaps(s, F[3], 2), lambda F: gaps(s, F[3], 1))
    c_id, p_id = hold["F"][0][1], hold["F"][1][1]
    s.g.edge(p_id, s.g.adj[c_id][0])
    for x, y in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (2, 2), (3, 0), (0, 3)):
        pair("sv_%d_%d" % (x, y), lambda F, x=x: gaps(s, F[3], x), lambda F, y=y: gaps(s, F[3], y))
    # the visited table: a slot taken by another id in the same pass, a full home bucket, two lanes after one slot
    # (radii above the bound: the ids are inserted and counted, the list stays as it is)
    far = iter(range(4089, 3990, -1))
    two = RM.same_bucket(s.g, 2)
    pair("taken", lambda F: [(next(far), two[0])], lambda F: [(next(far), two[1])])
    five = RM.same_bucket(s.g, 5)
    pair("fill_bucket", lambda F: [(next(far), i) for i in five[:4]], lambda F: [])
    pair("full", lambda F: [], lambda F: [(next(far), five[4])])
    two = RM.same_bucket(s.g, 2)
    pair("race", lambda F: [], lambda F: [(next(far), i) for i in two])
    s.drain(1)
    s.row("four_more", s.front(4))
    for _ in range(41):
        s.c_row("commit40_c", lambda F: [])
        s.p_row("commit40_p", s.front(2))
    _CACHE[("wide", ef)] = s
    return s


def small(ef):
    """ef 1 .. 4: rows of more keys than the list holds, on c and on p"""
    if ("small", ef) in _CACHE:
        return _CACHE[("small", ef)]
    s = FR.Script(ef)
    s.row("one_entry", [s.next_lattice()])
    s.row("fill", s.front(6))
    for kind in ("none",) * 4 + ("behind",) * 3:
        if len(s.unexp()) < 2:  # (ef 1 always: no runner-up, the rows only keep the walk going)
            s.row("refill", s.front(6))
            if ef == 1:
                continue
        if kind == "none":
            s.c_row("c_none", lambda F: [])
            s.p_row("p_many", s.front(6))
        else:
            # c's keys between p and the list's end (none at ef 2: p is the end), p's in front of everything
            s.c_row("c_behind", lambda F: [s.between(F[1], x) for x in s.cur[s.cur.index(F[1]) + 1:]])
            s.p_row("p_more", s.front(ef + 2))
    _CACHE[("small", ef)] = s
    return s


SCRIPTS = [("wide", ef) for ef in EFS_WIDE] + [("small", ef) for ef in EFS_SMALL]
WANT_WIDE = {"sv_0_0", "sv_1_0", "sv_0_1", "sv_1_1", "sv_2_1", "sv_2_2", "sv_3_0", "sv_0_3", "sv_16_16", "p_front",
             "tie_c_small", "tie_p_small", "c_pushes_p", "p_pushes_c", "p_pa", "p_ab", "p_at_b", "shared", "taken", "full",
             "race", "miss_then_fold", "fold_then_miss", "kept_fold", "commit40", "cut"}
WANT_SMALL = {"cut"}  # ef >= 2: the keys of a committed pass below the bound are more than the list takes


def graph_of(kind, ef):
    if kind == "overflow":
        return FR.graph_of("overflow", ef)
    return (wide if kind == "wide" else small)(ef).g


def handmade(kind, ef):
    """(oracle, rows, levels, queries, graph) -- queries[0] is q*, three noisy ones follow"""
    ck = ("handmade", kind, ef if kind != "overflow" else 0)
    if ck not in _CACHE:
        from oracle import oracle_py as O
        g = graph_of(kind, ef)
        rows = np.zeros((N, D), dtype=np.float32)
        rows[:, 0] = g.r
        lv = np.zeros(N, dtype=np.uint8)
        orc = O.OracleHNSW(M, 32, D, O.VEC_F32)
        orc.import_points(rows, lv)
        offs = np.zeros(N + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(g.adj[i]) for i in range(N)])
        flat = np.array([x for i in range(N) for x in g.adj[i]], dtype=np.uint32)
        orc.import_layer(0, np.arange(N, dtype=np.uint32), offs, flat)
        orc.set_ep(g.ep)
        noise = np.random.default_rng(7).standard_normal((3, D)).astype(np.float32)
        qs = np.concatenate([np.zeros((1, D), np.float32), noise * np.float32([[2.0 ** -10], [2.0 ** -3], [4.0]])])
        _CACHE[ck] = (orc, rows, lv, qs.astype(np.float32), g)
    return _CACHE[ck]


def replayed(kind, ef_laid, ef=None):
    """(list, counters, passes, status) of q* on the graph laid for ef_laid, searched with ef"""
    ef = ef_laid if ef is None else ef
    ck = ("replayed", kind, ef_laid, ef)
    if ck not in _CACHE:
        orc, _, _, qs, g = handmade(kind, ef_laid)
        dist = orc.distance_batch(qs[0], np.arange(N, dtype=np.uint32))
        assert np.array_equal(dist, g.r)  # distances to q* are the radii, by construction
        adj0 = {i: g.adj[i] for i in range(N)}
        _CACHE[ck] = replay(adj0, lambda ids: dist[ids], RM.entry_of(orc, qs[0]), ef)
    return _CACHE[ck]


def assert_states(kind, ef):
    """what the graph's rows promise, on the replay's passes for q*"""
    _, _, passes, status = replayed(kind, ef)
    assert status == "ok"
    got = states(passes, graph_of(kind, ef))
    if kind == "wide":
        want = WANT_WIDE
    elif kind == "small":
        want = WANT_SMALL if ef >= 2 else set()
        assert (ef >= 2) == any(r["fold"] for r in passes), (kind, ef)
    else:
        want = set()
        assert any(r["fold"] for r in passes), (kind, ef)
    assert want <= got, (kind, ef, sorted(want - got))
    return got


# ---- graphs of three passes: full rows, the visited limit, a NaN distance -------------------------------------------
# e's row holds the next pass's c (radius 100) and p (200) -- and, for the visited limit, K fillers far behind them, so
# that e's row goes through overflow passes as tests/test_gpu_visited_limit.py's does; c's and p's rows hold fresh ids
# behind p, so the pass commits p.

LIMIT = 3072  # ids the layer-0 table of a 2^12-slot launch takes (ef <= 112 at m = 16): three quarters of its slots


def g_three(n_c, n_p, fillers=0):
    g = RM.Graph(40 + n_c + n_p + fillers)
    e = g.node(3000)
    g.ep = e
    c, p = g.node(100), g.node(200)
    for x in (c, p):
        g.edge(e, x)
    for _ in range(fillers):
        g.edge(e, g.node(3500))
    g.info = dict(c=c, p=p, row_c=[g.node(300 + i) for i in range(n_c)], row_p=[g.node(400 + i) for i in range(n_p)])
    for y in g.info["row_c"]:
        g.edge(c, y)
    for y in g.info["row_p"]:
        g.edge(p, y)
    return g


def index_of(g, rows=None):
    """(oracle, rows, levels) of a graph; `rows` overrides the one-axis rows"""
    from oracle import oracle_py as O
    if rows is None:
        rows = np.zeros((N, D), dtype=np.float32)
        rows[:, 0] = g.r
    lv = np.zeros(N, dtype=np.uint8)
    orc = O.OracleHNSW(M, 32, D, O.VEC_F32)
    orc.import_points(rows, lv)
    offs = np.zeros(N + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(g.adj[i]) for i in range(N)])
    flat = np.array([x for i in range(N) for x in g.adj[i]], dtype=np.uint32)
    orc.import_layer(0, np.arange(N, dtype=np.uint32), offs, flat)
    orc.set_ep(g.ep)
    return orc, rows, lv


def full_rows():
    """c's and p's rows of 32 fresh ids each into a list of three entries: one merge of 64 survivors (the big merge's
    pad lands behind its 64th place), cut at ef = 64, taken whole at ef = 128"""
    if "full_rows" not in _CACHE:
        g = g_three(32, 32)
        _CACHE["full_rows"] = (g,) + index_of(g)
    return _CACHE["full_rows"]


VISITED = {"under": 3050, "by_p": 3060, "by_c": 3066}  # K fillers; c's row holds 5 fresh ids, p's row 10


def visited(which):
    """(graph, oracle, rows, levels, the (n_dist, n_exp, sum_deg, overflow?) the first 2^12-slot launch ends q* with).
    Before the pass of c and p the table holds 1 + K + 2 ids.  under: 3 068 ids after p's claims, no overflow.  by_p:
    3 068 after c's claims, 3 078 after p's: p's claims reach the limit, and the query ends with the counters of both
    expansions.  by_c: 3 074 after c's claims: the query ends there, p not committed."""
    ck = ("visited", which)
    if ck not in _CACHE:
        K = VISITED[which]
        g = g_three(5, 10, K)
        after_c, after_p = 1 + K + 2 + 5, 1 + K + 2 + 5 + 10
        assert 1 + K + 2 <= LIMIT
        if which == "under":
            assert after_p <= LIMIT
            want = None
        elif which == "by_p":
            assert after_c <= LIMIT < after_p
            want = (after_p, 3, (K + 2) + 5 + 10)  # (n_dist counts the entry point's distance as the table counts its id)
        else:
            assert LIMIT < after_c
            want = (after_c, 2, (K + 2) + 5)
        _CACHE[ck] = (g,) + index_of(g) + (want,)
    return _CACHE[ck]


def q_inf():
    """a query whose distance to every row is +inf -- (0 - inf)^2 in component 1 -- and NaN to a row whose component 1
    is +inf itself: inf - inf.  Keys then order by id alone."""
    q = np.zeros((1, D), dtype=np.float32)
    q[0, 1] = np.inf
    return q


def nan_case(side):
    """(graph, oracle, rows, levels, query, the (n_dist, n_exp, sum_deg) q ends with) for a NaN distance of a fresh
    neighbour of c ("c"), of the committed p ("p"), of both ("both": c's is met first) or of none ("clean").  All
    distances are +inf, so ids order the walk: e < c < p < c's row < p's row, which keeps every key of c behind p."""
    ck = ("nan", side)
    if ck not in _CACHE:
        g = RM.Graph(77)
        ids = iter(range(1000, 2000, 10))
        e = g.node(3000, next(ids))
        g.ep = e
        c, p = g.node(100, next(ids)), g.node(200, next(ids))
        g.edge(e, c)
        g.edge(e, p)
        row_c = [g.node(300 + i, next(ids)) for i in range(3)]
        row_p = [g.node(400 + i, next(ids)) for i in range(4)]
        for y in row_c:
            g.edge(c, y)
        for y in row_p:
            g.edge(p, y)
        rows = np.zeros((N, D), dtype=np.float32)
        rows[:, 0] = g.r
        victims = ([row_c[1]] if side in ("c", "both") else []) + ([row_p[2]] if side in ("p", "both") else [])
        rows[victims, 1] = np.inf
        dist = np.full(N, np.inf, dtype=np.float32)
        dist[victims] = np.nan
        adj0 = {i: g.adj[i] for i in range(N)}
        _, counters, passes, status = replay(adj0, lambda i: dist[i], (float("inf"), e), 64)
        assert status == ("ok" if side == "clean" else "nan") and passes[1]["c"] == c and passes[1]["p"] == p
        # the expansion that meets the NaN is counted whole; c's is met before p is committed
        want = {"c": (2 + 3, 2, 2 + 3), "both": (2 + 3, 2, 2 + 3), "p": (2 + 3 + 4, 3, 2 + 3 + 4), "clean": counters}[side]
        assert counters == want, (side, counters, want)
        _CACHE[ck] = (g,) + index_of(g, rows) + (q_inf(), counters)
    return _CACHE[ck]
