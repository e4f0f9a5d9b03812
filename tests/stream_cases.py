"""What tests/test_gpu_stream_contract.py runs: the small indexes, their expected values and the device-form calls with
their buffers in HBM.  A helper of the tests, no tests of its own and no pytest.

The contract under test is where and when the device-pointer entry points of include/hnsw_mi355x.h run, not what they
compute, so every expected value comes from where the value tests take theirs: the CPU oracle (plain form), the CPU
restatement of the filtered graph walk (tests/filtered_restate.py), the numpy restatements of the merge
(tests/partitioned_restate.py) and of the collapse (hnsw_rs_amd.grouped.group_by_label).  All comparisons are exact, on
the bit patterns of every output array.

Every call has two sets of inputs, `real` and `decoy` (two disjoint query sets whose plain answers differ for every
query, asserted when a fixture is made; other rows and ranges): a call that read its inputs before the stream reached
it answers `decoy`, one that wrote after the stream went on leaves poison."""
import functools
import math
import time

import numpy as np

import hnsw_rs_amd as H
from oracle import oracle_py as O
from oracle import restate_np as R
from tests import filtered_restate as FR
from tests.partitioned_restate import merge_restate
from tests.util import oracle_from_product, rand_vectors

MAX = 0xFFFFFFFF
NONE = H.MASK_NONE
N, D, M, EF_CONS = 3000, 36, 8, 16
NQ, TOPN, EF = 64, 10, 64
N_LABELS = 17
POISON = 0x5A5A5A5A  # (as a float 1.5e16, as an id beyond every index here)
SHARDS = 3
POOL, N_GROUPS, PER_GROUP = 64, 5, 2
INF_BITS = 0x7F800000

SEARCH_FORMS = ("plain", "set", "range", "ranges", "set_range")
FORMS = SEARCH_FORMS + ("group", "merge")


def unit(x):
    """rows of unit length in the arithmetic of the cosine option: float32, one left-to-right sum of squares"""
    s = np.zeros(x.shape[0], dtype=np.float32)
    for e in range(x.shape[1]):
        s = s + x[:, e] * x[:, e]
    return x / np.sqrt(s)[:, None]


def set_rows(n_points, seed=7):
    """the four rows of the mask set: about 50 % of the ids, about 2 %, none, all"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n_points) < 0.5, rng.random(n_points) < 0.02, np.zeros(n_points, dtype=bool),
                     np.ones(n_points, dtype=bool)])


class World:
    """one index with its labels, its mask set, its oracle and its restatement; `dead`: the ids marked deleted"""

    def __init__(self, index, stored, levels, rows_b, labels, dead=(), cosine=False):
        self.index, self.stored, self.levels, self.cosine = index, stored, levels, cosine
        self.rows_b, self.labels, self.dead = rows_b, labels, np.asarray(sorted(dead), dtype=np.int64)
        self.set = index.mask_set(rows_b)
        self.orc = oracle_from_product(index, stored, levels)
        layers = [index.get_layer(l).csr() for l in range(index.nb_layers())]
        self.ridx = R.Index.from_csr(stored, index.vec_kind, layers, int(index.params.ep))
        self.real = H.synth_rows(0, 0x5EED0002, 0, NQ, index.dim)
        self.decoy = H.synth_rows(0, 0x5EED0002, NQ, NQ, index.dim)
        self._want = {}

    def queries(self, which):
        return self.real if which == "real" else self.decoy

    def live(self):
        a = np.ones(self.index.len(), dtype=bool)
        a[self.dead] = False
        return a

    # ---- the keys of the filtered forms: rows and ranges per query, other ones for the decoy -------------------------
    def keys(self, form, which):
        """-> dict of uint32 arrays as the form takes them in HBM (mask_of [nq]; lo, hi [nq] or [nq, 3])"""
        i = np.arange(NQ) + (0 if which == "real" else 3)
        out = {}
        if form in ("set", "set_range"):
            # rows 0 and 3 and no row for most queries; rows 1 and 2 -- fewer ids than efSearch, or none: the walk never
            # fills its result set and meets every node, which the restatement takes a while to follow -- for two each
            cycle = np.array(([0, 3, NONE] * 11)[:32], dtype=np.uint32)
            cycle[9], cycle[21] = 1, 2
            out["mask_of"] = cycle[i % 32]
        if form in ("range", "set_range"):
            lo = (i * 5) % N_LABELS
            width = np.array([3, 16, 8, 5, 2, 12, 1, 7])[i % 8]
            width[i % 32 == 27] = 0  # one label
            if form == "range":
                width[i % 32 == 11] = -1  # lo > hi: the empty range
            out["lo"] = lo.astype(np.uint32)
            out["hi"] = np.maximum(lo + width, 0).astype(np.uint32)
            out["lo"][lo + width < 0] = 1  # (0 - 1 would be UINT32_MAX, every label: (1, 0) is empty as well)
        if form == "ranges":
            a, b = (i * 5) % N_LABELS, (i * 7 + 2) % N_LABELS
            out["lo"] = np.stack([a, b, np.ones_like(a)], axis=1).astype(np.uint32)
            out["hi"] = np.stack([a, b + i % 3, np.zeros_like(a)], axis=1).astype(np.uint32)  # the last: padding (1, 0)
        return out

    def allowed(self, form, which):
        """-> bool [nq, len]: the ids each query of the form may return (the deleted ones taken out)"""
        k, n = self.keys(form, which), self.index.len()
        lab = np.zeros(n, dtype=np.int64)
        lab[:self.labels.shape[0]] = self.labels
        ok = np.tile(self.live(), (NQ, 1))
        if "mask_of" in k:
            rows = np.zeros((self.rows_b.shape[0] + 1, n), dtype=bool)
            rows[:-1, :self.rows_b.shape[1]] = self.rows_b
            rows[-1] = True  # HNSW_MASK_NONE
            ok &= rows[np.where(k["mask_of"] == NONE, self.rows_b.shape[0], k["mask_of"]).astype(np.int64)]
        if "lo" in k:
            lo, hi = k["lo"].reshape(NQ, -1).astype(np.int64), k["hi"].reshape(NQ, -1).astype(np.int64)
            ok &= ((lab[None, None, :] >= lo[:, :, None]) & (lab[None, None, :] <= hi[:, :, None])).any(axis=1)
        return ok

    # ---- expected values -----------------------------------------------------------------------------------------------
    def want(self, form, which, n=TOPN, ef=EF):
        """-> (ids, distance bits, counts, stats) of a search form as uint32 arrays, computed once (ef other than EF: the
        plain form with nothing deleted only)"""
        key = (form, which, n, ef)
        if key not in self._want:
            Q = self.queries(which)
            Qr = unit(Q) if self.cosine else Q
            assert ef == EF or (form == "plain" and self.dead.size == 0)
            if form == "plain" and self.dead.size == 0:
                ids, dists, counts, st = self.orc.search_batch(Qr, n, ef)
                ids, dists, counts = np.array(ids, dtype=np.uint32), np.array(dists, dtype=np.float32), np.array(counts)
                bits = np.where(ids == MAX, np.uint32(INF_BITS), dists.view(np.uint32))
                stats = np.concatenate([np.asarray(st)[:, :3].astype(np.uint32), np.zeros((NQ, 1), dtype=np.uint32)], axis=1)
                got = (ids, bits, counts.astype(np.uint32), stats)
            else:
                got = self.walk(Qr, n, self.allowed(form, which) if form != "plain" else np.tile(self.live(), (NQ, 1)))
            for a in got:
                a.setflags(write=False)
            self._want[key] = got
        return self._want[key]

    def walk(self, Qr, n, ok, exact=False):
        """the restatement of the filtered graph walk (or of the exact path) per query -> the four arrays"""
        nq = Qr.shape[0]
        ids, bits = np.full((nq, n), MAX, dtype=np.uint32), np.full((nq, n), INF_BITS, dtype=np.uint32)
        counts, stats = np.zeros(nq, dtype=np.uint32), np.zeros((nq, 4), dtype=np.uint32)
        for q in range(nq):
            row = ok[q]
            if exact:
                r = FR.exact(self.ridx, Qr[q], n, np.flatnonzero(row))
            else:
                r = FR.graph(self.ridx, Qr[q], n, EF, lambda i, row=row: bool(row[i]))
                assert self.fits(r), "the walk would fill the visited table it is meant to fit"
            w_ids, w_d, c = FR.padded(r, n)
            ids[q], bits[q], counts[q], stats[q, :3] = w_ids, w_d.view(np.uint32), c, r["counters"]
        return ids, bits, counts, stats

    def fits(self, r):
        """the walk stays within the table a launch at efSearch 64 starts with (4096 slots, 75 %: 3072 ids, checked before
        each pass: a whole row may follow the check), so that no query is left to _finish"""
        return r["visited0"] + r["maxdeg0"] <= 3072

    def want_group(self, which):
        """the collapse of the plain search's pool-wide lists -> (ids, bits, labels, sizes, counts, stats)"""
        c = self.want("plain", which, POOL)
        g = H.group_by_label(c[0], c[1].view(np.float32), c[2], self.labels, N_GROUPS, PER_GROUP)
        return (g[0], g[1].view(np.uint32), g[2], g[3], g[4], c[3])

    def check_real_differs_from_decoy(self):
        """the two query sets are answered differently, query by query (what makes a stale read visible)"""
        a, b = self.want("plain", "real"), self.want("plain", "decoy")
        same = [q for q in range(NQ) if np.array_equal(a[0][q], b[0][q])]
        assert not same, "real and decoy expect the same ids for queries %s" % same


def build_index(kind, cosine=False, n=N, d=D, seed=1, m=M, ef_cons=EF_CONS):
    vs = H.synth_rows(0, 0x5EED0001 + seed, 0, n, d)  # (values on both sides of 0: the cosine order is not the L2 order)
    lv = O.draw_levels(n, m, seed)
    index = H.HNSW.new(m, ef_cons, d, kind)
    if cosine:
        index.set_option("metric_cosine", 1)
    index.insert_bulk(vs, 8, False, levels=lv)
    stored = np.stack([index.get_point(i).get_vals() for i in range(n)]) if cosine else vs
    return index, stored, lv


def labels_of(n):
    return (np.arange(n) % N_LABELS).astype(np.uint32)


def dead_ids(n=N, k=30, seed=11):
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


@functools.lru_cache(maxsize=None)
def world(kind, variant="base"):
    """the fixture of a vector kind: 'base', 'deleted' (a second copy of the index with 30 ids marked deleted) or
    'cosine' (an index of its own under the cosine option).  Built once, shared, left unchanged: a test that changes an
    index takes a clone."""
    if variant == "deleted":
        base = world(kind)
        index = base.index.clone()  # (carries the label column; the set is the clone's own)
        dead = dead_ids()
        index.mark_deleted(dead)
        w = World(index, base.stored, base.levels, base.rows_b, base.labels, dead)
    else:
        index, stored, lv = build_index(kind, cosine=variant == "cosine")
        labels = labels_of(N)
        index.set_labels(labels)
        w = World(index, stored, lv, set_rows(N), labels, cosine=variant == "cosine")
    w.check_real_differs_from_decoy()
    return w


CAPTURE_EF, CAPTURE_D, CAPTURE_M, CAPTURE_N = 256, 128, 16, 1500


@functools.lru_cache(maxsize=None)
def capture_boundary_world():
    """f32 rows of 128 values at m = 16 (rows of 32 slots): at ef = CAPTURE_EF, the largest the header promises to be
    capturable, the lean kernel runs with its widest list that takes no stream-ordered scratch (four registers; from ef 257
    on it takes six and a second visited level in HBM)"""
    n = CAPTURE_N
    index, stored, lv = build_index(H.VEC_F32, n=n, d=CAPTURE_D, seed=2, m=CAPTURE_M, ef_cons=32)
    return World(index, stored, lv, set_rows(n), labels_of(n))


# ---- the synthetic shard lists of the merge ---------------------------------------------------------------------------
def shard_lists(seed):
    """[S][NQ][TOPN] lists as three shards could return them: sorted by (bits, id) in their present part; shard 1 of
    query 7 repeats shard 0's list on the same global ids (a duplicated pair across shards); shard 2's list of query 5 is
    empty; query 9 has every list empty"""
    rng = np.random.default_rng(seed)
    S, n = SHARDS, TOPN
    ids = np.zeros((S, NQ, n), dtype=np.uint32)
    dists = np.zeros((S, NQ, n), dtype=np.float32)
    counts = np.zeros((S, NQ), dtype=np.uint32)
    for s in range(S):
        for q in range(NQ):
            c = 0 if q == 9 or (q == 5 and s == 2) else int(rng.integers(1, n + 1))
            loc = rng.choice(5 * n, n, replace=False).astype(np.uint32)
            d = rng.integers(0, 8, n).astype(np.float32) * np.float32(0.25)
            order = np.lexsort((loc[:c], d[:c].view(np.uint32)))
            loc[:c], d[:c] = loc[:c][order], d[:c][order]
            loc[c:], d[c:] = MAX, np.inf
            ids[s, q], dists[s, q], counts[s, q] = loc, d, c
    ids[1, 7], dists[1, 7], counts[1, 7] = ids[0, 7], dists[0, 7], counts[0, 7]
    stats = rng.integers(0, 2 ** 31, (S, NQ, 4)).astype(np.int64)
    stats[:, :, 3] = 0
    return ids, dists, counts, stats


MERGE_BASE = np.array([0, 0, 1000], dtype=np.uint32)  # shards 0 and 1 overlap: the same local id is the same point


def want_merge(lists, with_counts=True, with_stats=True):
    ids, dists, counts, stats = lists
    w = merge_restate(ids, dists, counts if with_counts else None, stats if with_stats else None, MERGE_BASE, None, TOPN)
    out = [w[0], w[1].view(np.uint32), w[2]]
    if with_stats:
        out.append(w[3].astype(np.uint32))
    return tuple(out)


def pool_lists(seed, n_labelled=N):
    """[NQ][POOL] candidate lists as a search leaves them, for the collapse: distinct ids below n_labelled, ascending
    distances, a count per query (query 9: none), a stats record"""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.choice(n_labelled, POOL, replace=False) for _ in range(NQ)]).astype(np.uint32)
    dists = np.sort(rng.random((NQ, POOL), dtype=np.float32), axis=1)
    counts = rng.integers(1, POOL + 1, NQ).astype(np.uint32)
    counts[9] = 0
    stats = rng.integers(0, 2 ** 31, (NQ, 4)).astype(np.int64)
    stats[:, 3] = 0
    return ids, dists, counts, stats


def want_collapse(lists, labels):
    ids, dists, counts, stats = lists
    g = H.group_by_label(ids, dists, counts, labels, N_GROUPS, PER_GROUP)
    return (g[0], g[1].view(np.uint32), g[2], g[3], g[4], stats.astype(np.uint32))


# ---- a graph whose walks fill the first visited table: what makes _finish re-run queries -----------------------------
RERUN_N, RERUN_D, RERUN_NQ = 5000, 12, 8


@functools.lru_cache(maxsize=None)
def rerun_world():
    """An imported random graph (six random links a node, symmetric: about 12 neighbours) with a hub: node 5 is joined to 3500 nodes.  The
    plain search of the hub's own vector expands the hub and meets more ids than the 3072 the first table (4096 slots)
    holds; under a filter that allows fewer than efSearch ids the result set never fills and the walk meets every node.
    Both fit the next table (8192 slots, 6144 ids): _finish re-runs them there and they end on the graph path."""
    n, d = RERUN_N, RERUN_D
    vs = rand_vectors(n, d, 81)
    rng = np.random.default_rng(82)
    nbrs = rng.integers(0, n, size=(n, 6))
    rows = [set() for _ in range(n)]
    for i in range(n):
        for j in nbrs[i].tolist():
            if j != i:
                rows[i].add(j)
                rows[j].add(i)
    for t in range(100, 3600):
        rows[5].add(t)
        rows[t].add(5)
    index = H.HNSW.new(4, None, d, H.VEC_QUANT8)
    index.import_points(vs, np.zeros(n, dtype=np.uint8))
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    index.import_layer(0, np.arange(n, dtype=np.uint32), offs, np.concatenate([np.array(sorted(r), dtype=np.uint32) for r in rows]))
    index.set_ep(0)
    labels = np.where(np.arange(n) % 97 == 0, 1, 0).astype(np.uint32)  # label 1: 52 ids, fewer than efSearch
    index.set_labels(labels)
    rows_b = np.stack([labels == 1, np.ones(n, dtype=bool)])
    w = RerunWorld(index, vs, np.zeros(n, dtype=np.uint8), rows_b, labels)
    w.real = rand_vectors(RERUN_NQ, d, 83)
    w.decoy = rand_vectors(RERUN_NQ, d, 84)
    w.real[0] = vs[5]
    w.decoy[0] = vs[5] + np.float32(0.01)
    return w


class RerunWorld(World):
    def fits(self, r):
        """the walk fits the second table (8192 slots, 6144 ids, checked before each pass of up to 64 ids)"""
        return r["visited0"] + 64 <= 6144

    def keys(self, form, which):
        one = np.ones(RERUN_NQ, dtype=np.uint32)
        out = {}
        if form in ("set", "set_range"):
            out["mask_of"] = 0 * one if form == "set" else one  # (row 0: the sparse one; with a range: row 1, everything)
        if form in ("range", "set_range"):
            out["lo"], out["hi"] = one.copy(), one.copy()
        if form == "ranges":
            out["lo"] = np.stack([one, one, one], axis=1)
            out["hi"] = np.stack([one, 0 * one, 0 * one], axis=1)
        return out

    def want(self, form, which, n=TOPN, ef=EF):
        assert ef == EF
        key = ("plain" if form == "plain" else "label 1", which, n)  # (every filtered form names the same 52 ids)
        if key not in self._want:
            Qr = self.queries(which)
            if form == "plain":
                ids, dists, counts, st = self.orc.search_batch(Qr, n, EF)
                stats = np.concatenate([np.asarray(st)[:, :3].astype(np.uint32), np.zeros((RERUN_NQ, 1), dtype=np.uint32)], axis=1)
                assert stats[0, 0] > 3072 + 64, "the hub's query does not fill the first table"
                got = (np.array(ids, dtype=np.uint32), np.array(dists, dtype=np.float32).view(np.uint32),
                       np.array(counts, dtype=np.uint32), stats)
            else:
                ok = np.tile((self.labels == 1)[None, :], (RERUN_NQ, 1))
                got = self.walk(Qr, n, ok)
                assert (got[3][:, 0] > 3072 + 64).all(), "a filtered walk does not fill the first table"
            self._want[key] = got
        return self._want[key]


# ---- the calls, with their buffers in HBM ------------------------------------------------------------------------------
def to_dev(torch, a):
    """a numpy array -> an int32 tensor in HBM holding its bits (float32 and uint32 alike)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.int64:
        a = a.astype(np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to(torch.device("cuda:0"))


class Call:
    """One device-form call: its inputs (each with the real and the decoy contents resident in HBM, so that switching
    them is a device-to-device copy that the host does not wait for) and its outputs, all int32 tensors of bits.
    enqueue(stream) makes the call; finish(stream) its _finish, where the form has one."""

    def __init__(self, torch, form, inputs, out_shapes, enqueue, finish=None):
        dev = torch.device("cuda:0")
        self.torch, self.form = torch, form
        self.src = {w: {k: to_dev(torch, v[i]) for k, v in inputs.items()} for i, w in enumerate(("real", "decoy"))}
        self.inp = {k: torch.empty_like(t) for k, t in self.src["real"].items()}
        self.out = {k: torch.empty(shape, dtype=torch.int32, device=dev) for k, shape in out_shapes.items()}
        self.copy = {k: torch.empty_like(t) for k, t in self.out.items()}
        self._enqueue, self._finish = enqueue, finish

    def distinguishable(self):
        """the premise of every case: the real and the decoy inputs are answered with different ids, so a read of stale
        inputs shows -> self"""
        a, b = self.want("real"), self.want("decoy")
        assert len(a) == len(b) == len(self.out), self.form
        assert not np.array_equal(np.asarray(a[0]), np.asarray(b[0])), "%s: real and decoy expect the same ids" % self.form
        return self

    def load(self, which):
        """(on the current torch stream) the inputs take the contents `which`"""
        for k, t in self.inp.items():
            t.copy_(self.src[which][k], non_blocking=True)

    def load_arrays(self, arrays):
        """(on the current torch stream, the host waits) the inputs take new contents from the host"""
        for k, a in arrays.items():
            self.inp[k].copy_(to_dev(self.torch, a))

    def poison(self):
        for t in self.out.values():
            t.fill_(POISON)

    def take(self):
        """(on the current torch stream) the outputs are copied aside and poisoned again"""
        for k, t in self.out.items():
            self.copy[k].copy_(t, non_blocking=True)
        self.poison()

    def enqueue(self, stream):
        self._enqueue(self.inp, self.out, stream)

    def finish(self, stream):
        self._finish(self.inp, self.out, stream)

    def arrays(self, copies=True):
        """the outputs (or their copies) on the host, uint32, in the order of the expected tuple"""
        return tuple(t.cpu().numpy().view(np.uint32) for t in (self.copy if copies else self.out).values())


SEARCH_OUT = lambda nq, n: {"ids": (nq, n), "dists": (nq, n), "counts": (nq,), "stats": (nq, 4)}  # noqa: E731


def search_call(torch, w, form, n=TOPN, ef=EF):
    """the device form `form` of world w over its real / decoy queries and keys, and what it must return for each"""
    index, s = w.index, w.set
    nq = w.real.shape[0]
    inputs = {"Q": (w.real, w.decoy)}
    kr, kd = w.keys(form, "real"), w.keys(form, "decoy")
    for k in kr:
        inputs[k] = (kr[k], kd[k])

    def args(i, o, stream):
        p = lambda t: t.data_ptr()  # noqa: E731
        mid = {"plain": (), "set": (s, i.get("mask_of")), "range": (i.get("lo"), i.get("hi")),
               "ranges": (3, i.get("lo"), i.get("hi")), "set_range": (s, i.get("mask_of"), i.get("lo"), i.get("hi"))}[form]
        if form == "plain":
            return (p(i["Q"]), nq, n, ef, p(o["ids"]), p(o["dists"]), p(o["counts"]), p(o["stats"]), stream)
        return (i["Q"], nq, n, ef) + mid + (o["ids"], o["dists"], o["counts"], o["stats"], stream)

    name = {"plain": "search_batch_device", "set": "search_batch_filtered_device",
            "range": "search_batch_filtered_range_device", "ranges": "search_batch_filtered_ranges_device",
            "set_range": "search_batch_filtered_set_range_device"}[form]
    call = Call(torch, form, inputs, SEARCH_OUT(nq, n),
                lambda i, o, st: getattr(index, name)(*args(i, o, st)),
                lambda i, o, st: getattr(index, name + "_finish")(*args(i, o, st)))
    call.want = lambda which: w.want(form, which, n, ef)
    return call.distinguishable()


def group_call(torch, w):
    """hnsw_group_by_label_device of world w over two sets of synthetic candidate lists"""
    lists = {"real": pool_lists(31), "decoy": pool_lists(32)}
    names = ("ids_in", "dists_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}
    shapes = {"ids": (NQ, N_GROUPS, PER_GROUP), "dists": (NQ, N_GROUPS, PER_GROUP), "labels": (NQ, N_GROUPS),
              "sizes": (NQ, N_GROUPS), "counts": (NQ,), "stats": (NQ, 4)}

    def enqueue(i, o, stream):
        w.index.group_by_label_device(NQ, POOL, N_GROUPS, PER_GROUP, i["ids_in"], i["dists_in"], i["counts_in"], i["stats_in"],
                                      o["ids"], o["dists"], o["labels"], o["sizes"], o["counts"], o["stats"], stream)

    call = Call(torch, "group", inputs, shapes, enqueue)
    call.want = lambda which: want_collapse(lists[which], w.labels)
    return call.distinguishable()


def merge_call(torch, with_counts=True, with_stats=True):
    """hnsw_merge_topk_device over two sets of synthetic shard lists"""
    lists = {"real": shard_lists(41), "decoy": shard_lists(42)}
    names = ("ids_in", "dists_in", "counts_in", "stats_in")
    inputs = {k: (lists["real"][j], lists["decoy"][j]) for j, k in enumerate(names)}
    shapes = {"ids": (NQ, TOPN), "dists": (NQ, TOPN), "counts": (NQ,)}
    if with_stats:
        shapes["stats"] = (NQ, 4)

    def enqueue(i, o, stream):
        H.merge_topk(SHARDS, NQ, TOPN, i["ids_in"], i["dists_in"], i["counts_in"] if with_counts else None,
                     i["stats_in"] if with_stats else None, MERGE_BASE, None, o["ids"], o["dists"], o["counts"],
                     o.get("stats"), stream)

    call = Call(torch, "merge", inputs, shapes, enqueue)
    call.want = lambda which: want_merge(lists[which], with_counts, with_stats)
    return call.distinguishable()


def make_call(torch, w, form):
    return group_call(torch, w) if form == "group" else merge_call(torch) if form == "merge" else search_call(torch, w, form)


def verdict(got, want, decoy=None):
    """None when every output array equals its expected one bit for bit, else what is wrong: stale inputs, late
    outputs, or plainly wrong ones.  decoy: a function that gives the expected values of the decoy inputs (asked only
    when something is wrong)"""
    def equal(exp):
        assert len(exp) == len(got), "%d expected arrays for %d outputs" % (len(exp), len(got))
        return all(np.array_equal(g, np.asarray(x).astype(np.uint32).reshape(g.shape)) for g, x in zip(got, exp))
    if equal(want):
        return None
    if decoy is not None and equal(decoy()):
        return "the outputs are those of the decoy inputs: the work ran ahead of the stream"
    if any((g == POISON).any() for g in got):
        return "poison survived in the outputs: the work ran behind the stream (or not at all)"
    bad = [k for k, (g, x) in enumerate(zip(got, want)) if not np.array_equal(g, np.asarray(x).astype(np.uint32).reshape(g.shape))]
    return "output arrays %s differ from the expected values" % bad


# ---- the gate ----------------------------------------------------------------------------------------------------------
GATE_FACTOR, GATE_MIN_S, GATE_MAX_S = 50, 0.050, 1.0
UNIT_CYCLES = 1000000


@functools.lru_cache(maxsize=None)
def gate_unit_seconds(torch):
    """the device time of one gate unit (torch.cuda._sleep of UNIT_CYCLES), measured with an event pair on an idle stream"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(UNIT_CYCLES)  # (the first launch loads the kernel)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(4):
            torch.cuda._sleep(UNIT_CYCLES)
        b.record(s)
    s.synchronize()
    return a.elapsed_time(b) / 4 / 1e3


def host_seconds(call, stream):
    """the median host time of the warmed call over 5 calls on the otherwise idle stream"""
    times = []
    for _ in range(5):
        stream.synchronize()
        t0 = time.perf_counter()
        call.enqueue(stream.cuda_stream)
        times.append(time.perf_counter() - t0)
    stream.synchronize()
    return sorted(times)[2]


def gate_cycles(torch, host_s):
    """the gate's length in cycles of torch.cuda._sleep: the larger of 50 x the call's host time and 50 ms (the factor
    guards against a descheduled host thread); more than 1 s is refused -> (cycles, seconds)"""
    unit_s = gate_unit_seconds(torch)
    assert unit_s > 0, "the gate unit takes no measurable device time"
    want_s = max(GATE_FACTOR * host_s, GATE_MIN_S)
    assert want_s <= GATE_MAX_S, ("the gate would exceed its cap of %.1f s: the call takes the host %.6f s, a gate unit "
                                  "takes the device %.6f s" % (GATE_MAX_S, host_s, unit_s))
    return int(math.ceil(want_s / unit_s * UNIT_CYCLES)), want_s
