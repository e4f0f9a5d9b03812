"""The small merge of the lean kernels' sorted list (search_lean.hip, Lst<R>::merge and LstHT::merge): a
merge of one or two survivors inserts them one at a time by shifting the list -- a compare of every entry against the
key, the same compare on the row of the entries before, two selects -- and cuts the list and refreshes its bound once,
behind the last key.  The fixtures and the CPU replay glue of tests/test_small_merge_host.py (no GPU) and
tests/test_gpu_small_merge.py.

Hand-made layer-0 graphs in the manner of tests/big_merge.py: tests/runner_up_miss.py's Graph class and one-axis rows
(the target query q* is the origin and row i is (r_i, 0, ..., 0): its distance to q* is the integer r_i exactly), one
layer, N = 8 192 ids, tests/big_merge.py's `merges` record.  One graph per ef, laid row by row by a Script that keeps a
model of the walk beside it: every row is given to the entry that is expanded next (the list's smallest unexpanded
one), so that row i of the script is merge i of the replay, and the radii of a row are chosen against the model's list
at that moment.  What a row's name promises is asserted on the replay's record (assert_pattern) before anything is
asked of a GPU:

  one_entry       one survivor into a list of one entry (at ef 1 that list is full: the survivor replaces it)
  fill            rows of up to 32 ids until the list holds ef - 1 entries
  to_full         one survivor into a list of ef - 1 entries: the list becomes full, its bound valid
  last            one survivor into a full list at entry ef - 1: it replaces the last
  front           ... in front of entry 0: every entry moves, the last falls off
  at63, at64      ... at entry 63 (the head's last entry is carried to the tail's front) and at entry 64 (the tail's
                  front, the head untouched); ef > 64
  two_head        two survivors below entry 63, entries between them
  two_across      one on each side of entries 63 / 64; ef >= 66
  two_tail        both beyond entry 63; ef >= 67
  two_adjacent    two survivors next to each other in the result
  vanish_lo, _hi  two survivors below the bound of which the larger is not below the bound the smaller sets: it lands
                  at place ef and the cut removes it.  The smaller key in the lower lane, and in the higher one
  tie_smaller_id, tie_larger_id   a survivor at the distance of an entry the list holds, sorting before and behind it
  tie_pair        two survivors of one merge at one distance
  front_expanded  a survivor in front of entries that are expanded: their flag travels with them (n_exp and the result
                  catch a re-expansion)
  front2, pc_a, pc_b   two survivors in front (the next pass's c and p), then c's row and the committed p's row of one
                  survivor each: a small merge of keys in lanes 32 .. 63 right after c's small merge; ef >= 3
  big3, after_big three survivors (the merge goes through LDS), then one: a small merge right after a big one
"""
import numpy as np

from tests import big_merge as BM
from tests import runner_up_miss as RM

D, M, S0, N, TOPN = RM.D, RM.M, RM.S0, RM.N, RM.TOPN
EFS = (1, 2, 3, 64, 65, 68, 128, 129, 256)  # Lst<1> (1 .. 64), LstHT (65, 68, 128), Lst<4> (129, 256)
E_RADIUS = 4090  # the entry point: above every other radius, the list's last entry until it is pushed off
merges = BM.merges

_CACHE = {}


class Script:
    """a graph laid row by row beside a model of the walk over it"""

    def __init__(self, ef):
        self.ef = ef
        self.g = RM.Graph(100 + ef)
        self.g.ep = self.g.node(E_RADIUS)
        self.cur = [(float(E_RADIUS), self.g.ep)]  # the model's list: (radius, id), ascending
        self.done = set()                          # expanded ids
        self.names = []                            # row i's name
        self.lattice = 991                         # the fill's radii, `space` apart: room for the rows' keys between them
        self.space = max(10, min(40, 3000 // ef))

    def holder(self):
        """the entry that is expanded next"""
        return next(k for k in self.cur if k[1] not in self.done)

    def row(self, name, nodes):
        """the next expansion's row: nodes = [(radius, id or None)] in lane order"""
        x = self.holder()[1]
        assert not self.g.adj[x] and len(nodes) <= S0
        self.done.add(x)
        keys = []
        for r, i in nodes:
            y = self.g.node(r, i)
            self.g.edge(x, y)
            keys.append((float(r), y))
        last = self.cur[self.ef - 1] if len(self.cur) >= self.ef else None
        self.cur = sorted(self.cur + [k for k in keys if last is None or k < last])[:self.ef]
        self.names.append(name)

    def below(self, k, n=1):
        """n unused integer radii below entry k's and above entry k - 1's, descending: a key there lands at k.  Spread
        over the gap, so that later rows find room between them."""
        hi = self.cur[k][0]
        lo = self.cur[k - 1][0] if k > 0 else 0.0
        step = max(1.0, min(8.0, (hi - lo - 1) // (n + 1)))
        if 0 < k == self.ef - 1:
            step = 1.0  # a key that replaces the last entry narrows the last gap: take as little of it as possible
        out = [(hi - step * (i + 1), None) for i in range(n)]
        assert out[-1][0] > lo, (self.ef, k, hi, lo)
        return out

    def next_lattice(self):
        self.lattice += self.space
        return (self.lattice, None)

    def fill(self, upto):
        while len(self.cur) < upto:
            k = min(S0, upto - len(self.cur))
            self.row("fill", [self.next_lattice() for _ in range(k)])

    def tied(self, k, smaller):
        """a key at entry k's radius with a smaller / a larger unused id"""
        r, i = self.cur[k]
        ids = range(i - 1, -1, -1) if smaller else range(i + 1, N)
        return [(r, next(j for j in ids if j not in self.g.used))]


def script(ef):
    if ("script", ef) in _CACHE:
        return _CACHE[("script", ef)]
    s = Script(ef)
    lo = lambda k: s.below(k)[0]
    s.row("one_entry", [s.next_lattice()])
    if ef >= 3:  # (at ef 2 the list of one entry is the list of ef - 1 entries)
        s.fill(ef - 1)
        s.row("to_full", [s.next_lattice()])
    assert len(s.cur) == ef
    s.row("last", s.below(ef - 1))
    s.row("front", s.below(0))
    if ef > 64:
        s.row("at63", s.below(63))
        s.row("at64", s.below(64))
    if ef >= 5:
        s.row("two_head", [lo(3), lo(1)])
    if ef >= 66:
        s.row("two_across", [lo(min(ef - 2, 65)), lo(10)])
        s.row("two_across", [lo(9), lo(min(ef - 2, 65))])
    if ef >= 67:
        s.row("two_tail", [lo(64), lo(min(ef - 2, 66))])
    if ef >= 2:
        s.row("two_adjacent", s.below(2 if ef >= 5 else 0, 2))
    b, a = s.below(ef - 1, 2)  # descending: a < b
    s.row("vanish_lo", [a, b])
    b, a = s.below(ef - 1, 2)
    s.row("vanish_hi", [b, a])
    s.row("tie_smaller_id", s.tied(min(ef - 1, 5), True))
    if ef >= 2:
        s.row("tie_larger_id", s.tied(min(ef - 2, 7), False))
        r = lo(12 if ef >= 64 else 0)[0]
        s.row("tie_pair", [(r, None), (r, None)])
        s.row("front_expanded", s.below(0))
    if ef >= 3:
        s.row("front2", s.below(0, 2))
        s.row("pc_a", s.below(ef - 1))
        s.row("pc_b", s.below(ef - 1))
    s.row("big3", [lo(ef - 1), lo(20), lo(30)] if ef >= 64 else s.below(0, 3))
    s.row("after_big", s.below(ef - 1))
    _CACHE[("script", ef)] = s
    return s


def handmade(ef, dim=D, kind=None):
    """(oracle, rows, levels, queries, script) of ef's graph -- queries[0] is q*, three noisy ones follow"""
    from oracle import oracle_py as O
    kind = O.VEC_F32 if kind is None else kind
    ck = ("handmade", ef, dim, kind)
    if ck not in _CACHE:
        s = script(ef)
        g = s.g
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
        _CACHE[ck] = (orc, rows, lv, qs.astype(np.float32), s)
    return _CACHE[ck]


def replayed(ef):
    """(list, counters, merges) of q* on ef's graph, f32 d = 100"""
    ck = ("replayed", ef)
    if ck not in _CACHE:
        orc, _, _, qs, s = handmade(ef)
        dist = orc.distance_batch(qs[0], np.arange(N, dtype=np.uint32))
        assert np.array_equal(dist, s.g.r)  # distances to q* are the radii, by construction
        adj0 = {i: s.g.adj[i] for i in range(N)}
        _CACHE[ck] = merges(adj0, lambda ids: dist[ids], RM.entry_of(orc, qs[0]), ef)
    return _CACHE[ck]


def expanded_at(ms):
    """per merge: the id whose row it merges (the first entry of the list before it that no merge before it took)"""
    done, out = set(), []
    for r in ms:
        x = next(k[1] for k in r["before"] if k[1] not in done)
        done.add(x)
        out.append(x)
    return out


def assert_pattern(ef, ms, s):
    """what the rows' names promise (module docstring), on the replay's merges for q*: merge i is row i"""
    assert len(ms) >= len(s.names), (ef, len(ms), len(s.names))
    who = expanded_at(ms)
    seen = set()
    for i, name in enumerate(s.names):
        r = ms[i]
        what = (ef, i, name, r["kind"], r["n_cur"], r["m"], r["pos"], r["n_new"])
        m, pos, full = r["m"], r["pos"], r["n_cur"] == ef
        seen.add(name)
        if name == "fill":
            assert r["n_cur"] < ef and m == r["fresh"], what
            continue
        if name == "one_entry":
            assert r["n_cur"] == 1 and m == 1 and r["n_new"] == min(2, ef), what
        if name == "to_full":
            assert r["n_cur"] == ef - 1 and m == 1 and r["n_new"] == ef, what
        if name in ("last", "pc_a", "pc_b", "after_big"):
            assert full and m == 1 and pos == [ef - 1], what
        if name in ("front", "front_expanded"):
            assert full and m == 1 and pos == [0], what
        if name == "front_expanded":
            moved = [k[1] for k in r["before"][:ef - 1]]  # entries that move up and stay
            assert any(x in set(who[:i + 1]) for x in moved), what
        if name == "at63":
            assert full and m == 1 and pos == [63], what
        if name == "at64":
            assert full and m == 1 and pos == [64], what
        if name == "two_head":
            assert full and m == 2 and pos[1] < 63 and pos[1] - pos[0] > 1, what
        if name == "two_across":
            assert full and m == 2 and pos[0] < 63 and 64 < pos[1] < ef, what
        if name == "two_tail":
            assert full and m == 2 and 64 <= pos[0] and pos[0] + 1 < pos[1] < ef, what
        if name == "two_adjacent":
            assert full and m == 2 and pos[1] == pos[0] + 1 < ef, what
        if name in ("vanish_lo", "vanish_hi"):
            assert full and m == 2 and pos == [ef - 1, ef] and r["n_new"] == ef, what
            first, second = (s.g.r[y] for y in s.g.adj[who[i]])  # lane order is row order
            assert (first < second) == (name == "vanish_lo"), what
        if name == "tie_smaller_id":
            assert full and m == 1 and pos[0] < ef, what
            held = r["before"][pos[0]]
            assert r["keys"][0][0] == held[0] and r["keys"][0][1] < held[1], what
        if name == "tie_larger_id":
            assert full and m == 1 and 0 < pos[0] < ef, what
            held = r["before"][pos[0] - 1]
            assert r["keys"][0][0] == held[0] and r["keys"][0][1] > held[1], what
        if name == "tie_pair":
            assert full and m == 2 and r["keys"][0][0] == r["keys"][1][0] and pos[1] < ef, what
        if name == "front2":
            assert full and m == 2 and pos == [0, 1], what
        if name == "pc_a":
            assert r["kind"] == "c", what
        if name == "pc_b":
            assert r["kind"] == "p" and s.names[i - 1] == "pc_a", what
        if name == "big3":
            assert full and m == 3, what
        if name == "after_big":
            assert ms[i - 1]["m"] >= 3, what
    # the two-sided row is laid twice: the smaller key in the lower lane and in the higher one
    want = {"one_entry", "last", "front", "vanish_lo", "vanish_hi", "tie_smaller_id", "big3", "after_big"}
    want |= {"two_adjacent", "tie_larger_id", "tie_pair", "front_expanded"} if ef >= 2 else set()
    want |= {"to_full", "front2", "pc_a", "pc_b"} if ef >= 3 else set()
    want |= {"two_head"} if ef >= 5 else set()
    want |= {"at63", "at64"} if ef > 64 else set()
    want |= {"two_across"} if ef >= 66 else set()
    want |= {"two_tail"} if ef >= 67 else set()
    assert want <= seen, (ef, sorted(want - seen))


# ---- the insertion by compare masks and selects, restated in numpy (what the kernel's small merge computes) ----------

INVALID = BM.INVALID
MASK = np.uint64(0x7FFFFFFFFFFFFFFF)  # LK_MASK: a key without its expanded flag
EXPANDED = np.uint64(1 << 63)


def insert_interleaved(L, e):
    """L: [64, R] registers of the interleaved list (entry i = register i % R of lane i / R) -> with e inserted.
    g = "this entry lies above e"; an entry above e takes the entry before it if that one lies above e too, else e.
    The entry before register r is register r - 1 of the same lane, before register 0 register R - 1 of the lane
    below; lane 0 has none and reads 0, which lies above nothing."""
    R = L.shape[1]
    below = np.concatenate([np.zeros(1, np.uint64), L[:-1, R - 1]])
    g = (L & MASK) > e
    gb = (below & MASK) > e
    # keys are unique and the list ascends: g is 0 .. 0 1 .. 1 over the entries, and the compare on the row before is
    # the same mask moved up by one entry
    assert np.array_equal(gb[1:], g[:-1, R - 1]) and not gb[0]
    flat = g.reshape(-1)
    assert not (flat[:-1] & ~flat[1:]).any()
    out = L.copy()
    for r in range(R - 1, -1, -1):
        frm = L[:, r - 1] if r > 0 else below
        gp = g[:, r - 1] if r > 0 else gb
        out[:, r] = np.where(g[:, r], np.where(gp, frm, e), L[:, r])
    return out


def insert_head_tail(L, e):
    """L: [64, 2] = head, tail (entry i = lane i of the head, entry 64 + i = lane i of the tail).  The entry before the
    tail's first is the head's last: the head's carry-out needs no case of its own."""
    head, tail = L[:, 0], L[:, 1]
    b0 = np.concatenate([np.zeros(1, np.uint64), head[:-1]])
    b1 = np.concatenate([head[63:], tail[:-1]])
    g0, p0 = (head & MASK) > e, (b0 & MASK) > e
    g1, p1 = (tail & MASK) > e, (b1 & MASK) > e
    assert np.array_equal(p0[1:], g0[:-1]) and not p0[0] and np.array_equal(p1[1:], g1[:-1]) and p1[0] == g0[63]
    # the carry by the issue's rule: x = g_63 ? entry_63 : e is what the tail's lane 0 takes whenever it takes anything
    x = head[63] if g0[63] else e
    out = np.stack([np.where(g0, np.where(p0, b0, e), head), np.where(g1, np.where(p1, b1, e), tail)], axis=1)
    if g1[0]:
        assert out[0, 1] == x
    return out


def small_merge(lst, n_cur, keys, ef, R, head_tail=False):
    """lst: 64 R u64 keys by entry (ascending without their flags, INVALID behind n_cur); keys: the wave's 64 u64 keys
    (INVALID = none).  -> (list by entry, n_new, the new bound), by the kernel's steps: the survivors in lane order,
    one insertion each, no test against the bound between them; then one cut at ef and one bound."""
    idx = BM.layout(R, head_tail)  # [lane, r] -> entry
    L = lst[idx]
    last = (lst[ef - 1] & MASK) if n_cur >= ef else INVALID
    surv = np.nonzero(keys < last)[0]
    for j in surv:
        L = insert_head_tail(L, keys[j]) if head_tail else insert_interleaved(L, keys[j])
    n_new = min(n_cur + len(surv), ef)
    L = np.where(idx >= ef, INVALID, L)
    out = np.empty(64 * R, dtype=np.uint64)
    out[idx] = L
    return out, n_new, ((out[ef - 1] & MASK) if n_new >= ef else INVALID)


def merge_model(lst, n_cur, keys, ef):
    """a plain sorted insert and truncate: the entries keep their flags, the order is that of the keys without them"""
    last = (lst[ef - 1] & MASK) if n_cur >= ef else INVALID
    allk = np.concatenate([lst[:n_cur], keys[keys < last]])
    allk = allk[np.argsort(allk & MASK, kind="stable")][:ef]
    return allk, len(allk)


def forms(ef):
    """(R, head + tail) of every list form that serves this ef: the one the kernels pick and the wider interleaved ones"""
    out = [(1, False)] if ef <= 64 else []
    out += [(2, True)] if 64 < ef <= 128 else []
    return out + [(R, False) for R in (4, 5, 8) if ef <= 64 * R]
