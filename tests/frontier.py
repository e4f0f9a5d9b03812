"""The frontier of the lean f32 kernels' list (search_lean.hip, Lst<1>::frontier and LstHT::frontier): the
keys of the first four unexpanded entries -- c, p and the two entries a, b behind them -- found once per pass by rank,
scatter and broadcast.  The pass takes c and p from it, commits p exactly when no fresh key of c sorts below p, and
requests the rows of a and b for the pass after unless a survivor of c's merge sorts in front of b.  The fixtures and
the CPU replay glue of tests/test_frontier_host.py (no GPU) and tests/test_gpu_frontier.py.

Hand-made layer-0 graphs in the manner of tests/small_merge.py (its Script: a graph laid row by row beside a model of
the walk; one-axis rows, so that the distance of row i to the target query q* is the integer r_i exactly).  The model
here also knows whose row comes next -- a pass's candidate c or its committed runner-up p -- so that a row can be given
to a pass's c with the frontier (c, p, a, b) of that pass in hand.  What a row's name promises is asserted on the
replay's passes (`states`) before anything is asked of a GPU:

  pa, ab            a survivor of c between p and a, between a and b: the pair behind p changes
  behind_b          ... exactly behind b: the pair stays
  tie_b_smaller, tie_b_larger   ... at b's distance with the smaller id (in front of b) and the larger (behind it)
  common_then_miss  a pass that takes a and b from its frontier, and c of the pass after puts a key below its runner-up
  commit40          p committed 40 times in a row: c's row empty, p's row two keys in front of everything (the pair
                    requested ahead is wrong every time)
  lone              one unexpanded entry at a pick (no runner-up); its row gives c in the head and p, a, b in the tail
                    (ef > 64), the next pass finds its only unexpanded entries in the tail
  push_off          c, p, a, b are the list's last four entries and c's two survivors push a and b off its end
  two, three        two and three unexpanded entries at a pick: no a, no b -- with and without survivors
and, at the end of every walk, no unexpanded entry at a pick.  `small` lays the same kinds of rows for ef 1 .. 4, where
the list is shorter than the frontier; tests/runner_up_miss.py's `overflow` gives a candidate and a runner-up whose row
carries an overflow pointer.
"""
import numpy as np

from tests import runner_up_miss as RM
from tests import small_merge as SM

D, M, S0, N, TOPN = RM.D, RM.M, RM.S0, RM.N, RM.TOPN
EFS_WIDE = (64, 65, 68, 128)  # Lst<1> at its widest, LstHT at one, four and sixty-four entries past the head
EFS_SMALL = (1, 2, 3, 4)
INF = (float("inf"), -1)

_CACHE = {}


# ---- the replay: the two-row pass with its frontier recorded ----------------------------------------------------------

def replay(adj0, dist_of, entry, ef, s0=S0):
    """tests/tools/miss_sim.replay with the frontier's view of every pass.  -> (list, (n_dist, n_exp, sum_deg), passes);
    a pass is a dict: F (the first four unexpanded keys at the pick, fewer where the list has fewer), n_unexp (all of
    them), cpos / ppos (entries of c and p), ordinary (a runner-up, and neither row beyond s0 slots), ovf_c / ovf_p,
    below (fresh keys of c below p), hit (p committed); of a hit: surv (c's survivors, ascending), common (none of them
    sorts in front of min(b, the bound before the merge)), after (the first three unexpanded keys after c's merge: p and
    the pair behind it), a_left / b_left (a, b pushed off the list by c's merge), n (entries before c's merge)."""
    import bisect
    ef = max(1, ef)
    sel, expanded, visited = [entry], set(), {entry[1]}
    counters = [0, 0, 0]

    def unexp(k=None):
        out = [e for e in sel if e[1] not in expanded]
        return out if k is None else out[:k]

    def expand(node):
        expanded.add(node)
        nbrs = [int(x) for x in adj0[node]]
        fresh = list(dict.fromkeys(n for n in nbrs if n not in visited))
        visited.update(fresh)
        counters[0] += len(fresh)
        counters[1] += 1
        counters[2] += len(nbrs)
        return [(float(d), n) for d, n in zip(dist_of(fresh), fresh)] if fresh else []

    def merge(keys):
        last = sel[ef - 1] if len(sel) >= ef else INF
        surv = sorted(k for k in keys if k < last)
        for k in surv:
            bisect.insort(sel, k)
        del sel[ef:]
        return surv, last

    passes = []
    while True:
        u = unexp()
        if not u:
            passes.append(dict(F=[], n_unexp=0, end=True))
            break
        F = u[:4]
        c, p = F[0], (F[1] if len(F) > 1 else None)
        ovf_c, ovf_p = len(adj0[c[1]]) > s0, p is not None and len(adj0[p[1]]) > s0
        rec = dict(F=F, n_unexp=len(u), cpos=sel.index(c), ppos=None if p is None else sel.index(p), c=c[1],
                   p=None if p is None else p[1], ovf_c=ovf_c, ovf_p=ovf_p, ordinary=p is not None and not ovf_c and not ovf_p,
                   hit=False, end=False, n=len(sel))
        keys = expand(c[1])
        rec["below"] = sorted(k for k in keys if p is not None and k < p)
        surv, last = merge(keys)
        passes.append(rec)
        if not rec["ordinary"]:
            continue
        nxt = unexp(3)
        if nxt and nxt[0] == p:
            b = F[3] if len(F) > 3 else INF
            rec.update(hit=True, surv=surv, common=not any(k < min(b, last) for k in surv), after=nxt,
                       a_left=len(F) > 2 and F[2] not in sel, b_left=len(F) > 3 and F[3] not in sel, sel_after=list(sel))
            merge(expand(p[1]))
    return sel, tuple(counters), passes


def check_rules(passes, what=""):
    """The two rules the kernel rests on.  Step 3: an ordinary pass commits p exactly when no fresh key of c is below p.
    Step 4: when no survivor of c sorts in front of min(b, the bound before the merge), the two unexpanded entries behind
    p after the merge are the frontier's a and b (as far as it has them).  -> the passes each was checked on"""
    n3 = n4 = 0
    for i, r in enumerate(passes):
        if r["end"] or not r["ordinary"]:
            continue
        assert r["hit"] == (not r["below"]), (what, i, r)
        n3 += 1
        if r["hit"] and r["common"]:
            assert r["after"][0] == r["F"][1] and r["after"][1:] == r["F"][2:4], (what, i, r)
            n4 += 1
    return n3, n4


def states(passes, ef):
    """the names of the module docstring that the passes of one walk show"""
    out = set()
    run = 0
    for i, r in enumerate(passes):
        out.add("unexp%d" % r["n_unexp"] if r["n_unexp"] < 4 else "unexp4+")
        if r["end"]:
            continue
        if r["cpos"] >= 64:
            out.add("tail_only")
        if r["ppos"] is not None:
            out.add("both_tail" if r["cpos"] >= 64 else ("c_head_p_tail" if r["ppos"] >= 64 else "both_head"))
        out |= ({"ovf_c"} if r["ovf_c"] else set()) | ({"ovf_p"} if r["ovf_p"] else set())
        run = run + 1 if r["hit"] else 0
        if run >= 40:
            out.add("commit40")
        if not r["hit"]:
            continue
        F, surv, sel = r["F"], r["surv"], r["sel_after"]
        if r["a_left"] and r["b_left"]:
            out.add("push_off")
        if len(F) == 2:
            out.add("no_a_surv" if surv else "no_a_nosurv")
        if len(F) == 3:
            out.add("no_b_surv" if surv else "no_b_nosurv")
        if len(F) == 4:
            p, a, b = F[1:]
            out |= {"surv_pa"} if any(p < k < a for k in surv) else set()
            out |= {"surv_ab"} if any(a < k < b for k in surv) else set()
            if b in sel and sel.index(b) + 1 < len(sel) and sel[sel.index(b) + 1] in surv:
                out.add("surv_behind_b")
            out |= {"tie_b_smaller"} if any(k[0] == b[0] and k[1] < b[1] for k in surv) else set()
            out |= {"tie_b_larger"} if any(k[0] == b[0] and k[1] > b[1] for k in surv) else set()
            nx = passes[i + 1]
            if r["common"] and not nx["end"] and nx["ordinary"] and not nx["hit"] and (nx["c"], nx["p"]) == (a[1], b[1]):
                out.add("common_then_miss")
        out.add("step4_common" if r["common"] else "step4_fallback")
    return out


# ---- the scripts ------------------------------------------------------------------------------------------------------

class Script(SM.Script):
    """tests/small_merge.py's Script that also knows whose row the next one is: 'c' (a pass's candidate) or 'p' (its
    runner-up, committed because c's row put nothing below it)"""

    def __init__(self, ef):
        super().__init__(ef)
        self.g = RM.Graph(300 + ef)
        self.g.ep = self.g.node(SM.E_RADIUS)
        self.cur = [(float(SM.E_RADIUS), self.g.ep)]
        self.phase = "c"
        self.front_r = 980  # radii in front of every lattice entry, handed out downwards

    def unexp(self):
        return [k for k in self.cur if k[1] not in self.done]

    def row(self, name, nodes):
        u = self.unexp()
        p = u[1] if self.phase == "c" and len(u) > 1 else None
        super().row(name, nodes)
        if self.phase == "p" or p is None:
            self.phase = "c"
        else:
            keys = [(float(self.g.r[y]), y) for y in self.g.adj[u[0][1]]]
            self.phase = "c" if any(k < p for k in keys) else "p"

    def c_row(self, name, nodes_of):
        """the next pass's c takes the row nodes_of(frontier); an empty row for a runner-up in between"""
        if self.phase == "p":
            self.row("idle_p", [])
        self.row(name, nodes_of(self.unexp()[:4]))

    def p_row(self, name, nodes):
        assert self.phase == "p", name
        self.row(name, nodes)

    def between(self, x, y):
        """an unused integer radius strictly between two keys' radii"""
        taken = {float(self.g.r[i]) for i in self.g.used}
        for r in range(int(x[0]) + 1, int(y[0])):
            if float(r) not in taken:
                return (r, None)
        raise AssertionError(("no room between", x, y))

    def after(self, k):
        """the entry behind key k in the model's list"""
        return self.cur[self.cur.index(k) + 1]

    def spread(self, k, n):
        """n unused integer radii between entries k - 1 and k with room between any two of them, descending"""
        hi, lo = self.cur[k][0], self.cur[k - 1][0]
        step = (hi - lo) // (n + 1)
        assert step >= 2, (self.ef, k, hi, lo)
        return [(hi - step * (i + 1), None) for i in range(n)]

    def roomy(self, n):
        """the last entry with room for n spread radii in front of it, all of which stay in a full list"""
        return next(k for k in range(len(self.cur) - n, 0, -1) if self.cur[k][0] - self.cur[k - 1][0] >= 2 * (n + 1))

    def front(self, n):
        out = []
        for _ in range(n):
            self.front_r -= 5  # (room for keys between two of them)
            out.append((self.front_r, None))
        return out

    def drain(self, leave):
        """rows that add nothing until `leave` unexpanded entries are left and the next row is a candidate's.  An empty
        row takes one entry and changes whose row is next; where that would end on a runner-up's row, a candidate's row
        puts one key in front of everything instead (a miss: the next row is a candidate's again)."""
        for _ in range(4 * self.ef + 8):
            u = len(self.unexp())
            if self.phase == "c" and u == leave:
                return
            assert u >= max(leave, 1), (self.ef, leave, u)
            if self.phase == "c" and (u - leave) % 2 == 1 and u >= 2:
                self.row("drain_miss", self.front(1))
            else:
                self.row("drain", [])
        raise AssertionError((self.ef, leave))


def wide(ef):
    """the script for a list of at least 64 entries"""
    if ("wide", ef) in _CACHE:
        return _CACHE[("wide", ef)]
    s = Script(ef)
    s.row("one_entry", [s.next_lattice()])
    s.fill(ef)
    assert len(s.cur) == ef and len(s.unexp()) >= 40
    s.c_row("pa", lambda F: [s.between(F[1], F[2])])
    s.c_row("ab", lambda F: [s.between(F[2], F[3])])
    s.c_row("behind_b", lambda F: [s.between(F[3], s.after(F[3]))])
    s.c_row("tie_b_smaller", lambda F: [(F[3][0], next(j for j in range(F[3][1] - 1, -1, -1) if j not in s.g.used))])
    s.c_row("tie_b_larger", lambda F: [(F[3][0], next(j for j in range(F[3][1] + 1, N) if j not in s.g.used))])
    # a and b taken from the frontier, then -- they are the next pass's c and p -- a key of c's below p
    s.c_row("common", lambda F: [s.between(F[3], s.after(F[3]))])
    s.p_row("idle_p", [])
    s.c_row("then_miss", lambda F: [s.between(F[0], F[1])])
    # down to one unexpanded entry; its row: c in the head, p, a and b in the list's last three places
    s.drain(1)
    s.row("lone", s.front(1) + s.spread(ef - 4, 3))  # (the key in front moves the three to the end)
    s.c_row("head_and_tail", lambda F: [])
    s.p_row("idle_p", [])
    # a, b are the only unexpanded entries (in the tail where there is one); b's row: the list's last four entries
    s.c_row("tail_only", lambda F: [])
    s.p_row("last_four", s.spread(ef - 4, 4))
    s.c_row("push_off", lambda F: [s.between(F[1], F[2]), s.between(F[1], F[2])])  # (two ids at one radius)
    s.p_row("idle_p", [])
    s.c_row("two", lambda F: [])                              # the two survivors: no a, no b
    s.p_row("three_more", s.spread(s.roomy(3), 3))
    s.c_row("three", lambda F: [])                            # c, p, a: no b, no survivor
    s.p_row("three_again", s.spread(s.roomy(3), 3))           # (they push a off the end)
    s.c_row("three_surv", lambda F: [s.between(F[1], F[2])])  # ... and a survivor between p and a
    s.drain(1)
    s.row("four_more", s.front(4))
    for _ in range(41):
        s.c_row("commit40_c", lambda F: [])
        s.p_row("commit40_p", s.front(2))
    _CACHE[("wide", ef)] = s
    return s


def small(ef):
    """ef 1 .. 4: the list is shorter than the frontier"""
    if ("small", ef) in _CACHE:
        return _CACHE[("small", ef)]
    s = Script(ef)
    s.row("one_entry", [s.next_lattice()])
    s.row("fill", s.front(6))  # more keys than the list takes
    for _ in range(3):
        s.row("front2", s.front(2))
    s.c_row("miss", lambda F: s.front(1))
    s.c_row("last", lambda F: s.below(ef - 1))
    s.c_row("more", lambda F: s.front(3))
    s.c_row("tie", lambda F: s.tied(0, False) + s.tied(0, True))
    # every count of unexpanded entries the list can hold, at a pick
    for leave in (3, 2, 1):
        if leave <= ef:
            s.row("full_row", s.front(8))  # (whoever's row it is: the list is all new keys afterwards)
            s.drain(leave)
            s.row("left%d" % leave, [])
    _CACHE[("small", ef)] = s
    return s


SCRIPTS = [("wide", ef) for ef in EFS_WIDE] + [("small", ef) for ef in EFS_SMALL]
# what every wide script's replay must show (module docstring), and what only a list with a tail can
WANT_WIDE = {"unexp0", "unexp1", "unexp2", "unexp3", "unexp4+", "surv_pa", "surv_ab", "surv_behind_b", "tie_b_smaller",
             "tie_b_larger", "common_then_miss", "commit40", "push_off", "no_a_nosurv", "no_b_nosurv", "no_b_surv",
             "step4_common", "step4_fallback", "both_head"}
WANT_TAIL = {"tail_only", "c_head_p_tail", "both_tail"}
WANT_OVERFLOW = {"ovf_c", "ovf_p"}


def graph_of(kind, ef):
    if kind == "overflow":
        if "overflow" not in _CACHE:
            _CACHE["overflow"] = RM.g_overflow()
        return _CACHE["overflow"]
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


def replayed(kind, ef):
    """(list, counters, passes) of q* on the graph"""
    ck = ("replayed", kind, ef)
    if ck not in _CACHE:
        orc, _, _, qs, g = handmade(kind, ef)
        dist = orc.distance_batch(qs[0], np.arange(N, dtype=np.uint32))
        assert np.array_equal(dist, g.r)  # distances to q* are the radii, by construction
        adj0 = {i: g.adj[i] for i in range(N)}
        _CACHE[ck] = replay(adj0, lambda ids: dist[ids], RM.entry_of(orc, qs[0]), ef)
    return _CACHE[ck]


def assert_states(kind, ef):
    """what the graph's rows promise, on the replay's passes for q*"""
    _, _, passes = replayed(kind, ef)
    check_rules(passes, (kind, ef))
    got = states(passes, ef)
    if kind == "wide":
        # (a tail of one entry, ef 65, cannot hold both c and p)
        want = WANT_WIDE | (WANT_TAIL - ({"both_tail"} if ef == 65 else set()) if ef > 64 else set())
    elif kind == "overflow":
        want = WANT_OVERFLOW
    else:
        want = {"unexp0", "unexp1"} | ({"unexp%d" % k for k in range(2, ef + 1) if k < 4}) | ({"unexp4+"} if ef >= 4 else set())
    assert want <= got, (kind, ef, sorted(want - got))
    return got


# ---- the routines, restated in numpy (what the kernel computes) -------------------------------------------------------

INVALID = SM.INVALID
MASK = SM.MASK
EXPANDED = SM.EXPANDED
SIGN = np.uint64(1 << 63)


def mbcnt(mask):
    """per lane: the set bits of a 64-lane mask below the lane"""
    return np.concatenate([[0], np.cumsum(mask.astype(np.int64))[:-1]])


def frontier(regs):
    """regs: the list's registers, [64] (one register: entry i = lane i) or [2, 64] (head, tail).  An entry is unexpanded
    when its sign bit is clear (INVALID has it set); its rank is the mbcnt of the ballot, the tail's ranks start at the
    head's count; ranks 0 .. 3 write their key at their rank into four places preset to INVALID; every lane reads the
    four.  -> [4] keys"""
    regs = np.atleast_2d(regs)
    slots = np.full(4, INVALID, dtype=np.uint64)  # the pad write
    base = 0
    for reg in regs:
        u = (reg & SIGN) == 0
        rank = mbcnt(u) + base
        w = u & (rank < 4)
        assert len(set(rank[w])) == int(w.sum())  # no two lanes write one place
        slots[rank[w]] = reg[w]
        base += int(u.sum())
    return slots


def commits(keys_c, pkey):
    """step 3: p is next exactly when no fresh key of c is below its key (the ballot of the foreseen miss is empty)"""
    return not (keys_c < pkey).any()


def pair_stays(keys_c, bkey, last_before):
    """step 4: a and b stay the pair behind p when no key of c is below min(b, the bound before the merge)"""
    return not (keys_c < min(bkey, last_before)).any()
