"""A state machine over the side tables of a handle: the deleted mask (deleted.h), the label column with its sorted
planner copy (labels.h) and the resident mask sets with their per-row caches (mask_set.h).  A helper of the tests, no
tests of its own (tests/test_update_machine_host.py, tests/test_gpu_update_machine.py).

Model     plain numpy and Python, written from the contracts in include/hnsw_mi355x.h, deleted.h, labels.h and
          mask_set.h; it never calls the library.  Answer state (vectors, deleted, labels, mask sets), transport state
          per HBM copy (Copy: exists, capacity, dirty words -- HbmWords restated) and cache state (what a mask row's count
          and list, and the label column's sort, were made for).  It predicts, for every call, the words each copy
          uploads and the recounts and compactions of the sets, and notes every transition it goes through (Model.ev).
schedule  schedule(seed, kind) -> a list of ops, each with the check that follows it; drawn from
          np.random.default_rng alone (the generator runs a Model of its own to draw valid ids), never from a product
          result, so a list can be replayed, cut to a prefix and run through the model without a GPU.
Machine   drives the product and the model through a schedule: product None (the model alone), "host" (the library with
          every GPU call skipped) or "gpu" (everything).  After every op the host-visible state is held to the model;
          on the GPU one drawn search family is then held to the CPU restatements (tests/filtered_restate.py,
          oracle/restate_np.py, the oracle) under the model's predicate, and the upload / recount counters to the model.
replay    replay(seed, kind, upto) re-runs the first `upto` ops: a failure names its step, the prefix is found by hand.
composite schedule(..., families="composite") keeps the ops and draws the checks from the search-then-post-process entry
          points (radius, diverse, from_rows / by_id, multi, late: COMPOSITE_FAMILIES) and two anchors.  A composite check
          predicts the candidate lists as check_grouped does, passes them through the feature's own restatement
          (hnsw_rs_amd.radius / diverse / from_rows / multi / late) and holds ids, distance / score / gap bits, counts,
          stats, the upload counters and the per-feature counters to it (Machine.check_composite).  What its lists go
          through is noted twice: as the model alone predicts it, and, product "host" or "gpu", as the restated lists show
          it ("seen:"; the graph is the host's, no GPU is needed for that).
"""
import collections
import hashlib
import os
import shutil
import tempfile
import threading

import numpy as np

NONE = -1
MAX = 0xFFFFFFFF
FULL = (0, MAX)
D, M, EF_CONS, N0 = 28, 8, 32, 120
HUGE = 10 ** 9
SEEDS, STEPS = (1, 2, 3), 160  # the committed schedules (tests/test_update_machine_host.py holds them to their coverage)
DEFAULT_EXACT_MAX, DEFAULT_CACHE_MB = 65536, 64

COUNTERS = ("deleted_mask_words_uploaded", "label_words_uploaded", "mask_set_words_uploaded", "mask_set_recounts",
            "mask_set_compactions", "uploads", "point_patches", "patch_fallbacks")
HOST_FAMILIES = ("count_labels", "set_count_read", "deleted_ids", "get_labels")
DEVICE_FAMILIES = ("set_device", "range_device", "set_range_device")
SEARCH_FAMILIES = ("search_batch", "filtered", "multi", "set", "range", "ranges", "set_range") + DEVICE_FAMILIES + \
    ("one", "one_threads", "grouped", "grouped_range", "grouped_row", "brute_force")
# every search family but the scan can take the graph path; the device forms plan nothing and never take the exact one,
# and the unfiltered entry points take it only under deletions (not required of a schedule)
PATH0_FAMILIES = tuple(f for f in SEARCH_FAMILIES if f != "brute_force")
PATH1_FAMILIES = ("filtered", "multi", "set", "range", "ranges", "set_range", "one", "one_threads", "grouped_range",
                  "grouped_row")
# the search-then-post-process entry points (lists_host.h) have schedules of their own: schedule(..., families="composite")
# draws its checks from these and the two anchors, and leaves every draw of the committed schedules where it is
COMPOSITE_SEEDS, COMPOSITE_STEPS = (11, 12), 150
COMPOSITE_FAMILIES = ("radius", "diverse", "diverse_range", "diverse_row", "from_rows", "by_id", "multi_vec", "late")
ANCHORS = ("search_batch", "brute_force")
FILTERED_COMPOSITES = ("diverse_range", "diverse_row")  # the host form whatever is deleted: their candidates are filtered
FEATURE_COUNTERS = ("radius_calls", "radius_rungs", "radius_launches", "diverse_calls", "diverse_launches",
                    "from_rows_calls", "from_rows_compose_launches", "from_rows_drop_launches", "multi_calls",
                    "multi_fuse_launches", "late_calls", "late_launches")
HOST_POOLS, DEVICE_POOLS, REFUSED_POOL = (8, 24, 64), (8, 64, 65, 200), 65
FUSE_MAX_CANDS, LATE_MAX_CANDS = 256, 1024  # (HNSW_FUSE_MAX_CANDS, HNSW_LATE_MAX_CANDS: T * pool of a call)
SURE = 3  # the model's nearest live rows of a vector, in float64: candidates of its list whatever the graph walk does


def words_of(n_bits):
    return (int(n_bits) + 63) // 64


# ---- the model --------------------------------------------------------------------------------------------------
class Copy:
    """HbmWords (deleted.h), restated: the HBM copy of host words.  sync(nw, slack) -> the words that travel: a whole
    copy of nw when there is no copy yet or d_cap < nw (the copy is made afresh with room for `slack` more words) or
    dirty * 8 > nw; otherwise exactly the dirty words; nothing dirty: 0."""

    def __init__(self, name, ev):
        self.name, self.ev = name, ev
        self.exists, self.cap, self.dirty, self.last_nw = False, 0, set(), None

    def touch(self, w):
        self.dirty.add(int(w))

    def sync(self, nw, slack):
        grown = self.exists and self.last_nw is not None and nw > self.last_nw
        had_dirty = bool(self.dirty)
        outcome = None
        if self.exists and self.cap < nw:  # outgrown: released and made afresh, whether or not a word is listed
            self.exists, outcome = False, "regrow"
            self.ev["%s:regrow_%s" % (self.name, "dirty" if had_dirty else "clean")] += 1
        if not self.exists:
            self.exists, self.cap = True, max(1, nw + slack)
            n, outcome = nw, outcome or "first"
        elif not self.dirty:
            n, outcome = 0, "clean"
        elif len(self.dirty) * 8 > nw:
            n, outcome = nw, "whole"
        else:
            n, outcome = len(self.dirty), "scatter"
        self.ev["%s:%s" % (self.name, outcome)] += 1
        if grown and outcome != "regrow":
            self.ev["%s:grown_within_%s" % (self.name, "dirty" if had_dirty else "clean")] += 1
        self.dirty.clear()
        self.last_nw = nw
        return n


class Cache:
    """what is valid for three keys (a mask row: row version, del version, len; the label sort: column version, del
    version, len).  use(key) -> whether it had to be made again; the transition is noted"""

    def __init__(self, name, key_names, ev):
        self.name, self.key_names, self.ev, self.key = name, key_names, ev, None

    def use(self, key):
        if self.key == key:
            self.ev["%s:reused" % self.name] += 1
            return False
        if self.key is None:
            self.ev["%s:first" % self.name] += 1
        else:
            moved = [n for n, a, b in zip(self.key_names, self.key, key) if a != b]
            self.ev["%s:killed_%s" % (self.name, moved[0] if len(moved) == 1 else "several")] += 1
        self.key = key
        return True


class SetModel:
    """hnsw_mask_set (mask_set.h): rows x allow_bits bools with a fixed allow_bits, the HBM copy, the row caches"""

    def __init__(self, bits, ev):
        self.bits = np.array(bits, dtype=bool).reshape(len(bits), -1)
        self.G, self.allow_bits = self.bits.shape
        self.W, self.ev = words_of(self.allow_bits), ev
        self.copy = Copy("set", ev)
        self.version = [1] * self.G
        self.cache = [Cache("row", ("version", "del", "len"), ev) for _ in range(self.G)]
        self.list_valid, self.d_cap = [False] * self.G, [0] * self.G
        self.list_bytes = 0
        # (create stores the rows it is given and lists their nonzero words; there is no copy yet)
        for g in range(self.G):
            for w in np.flatnonzero(self._row_words(g)):
                self.copy.touch(g * self.W + int(w))

    def _row_words(self, g, row=None):
        row = self.bits[g] if row is None else row
        padded = np.zeros(self.W * 64, dtype=bool)
        padded[: self.allow_bits] = row
        return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8")

    def words(self, g):
        return self._row_words(g).astype(np.uint64)

    def update(self, g, ids, allow):
        changed = False
        for i in ids:
            if bool(self.bits[g, i]) != bool(allow):
                self.bits[g, i] = bool(allow)
                self.copy.touch(g * self.W + (int(i) >> 6))
                changed = True
        if changed:
            self.version[g] += 1
        else:
            self.ev["noop:set"] += 1

    def write(self, g, row):
        row = np.asarray(row, dtype=bool)
        diff = np.flatnonzero(self._row_words(g) != self._row_words(g, row))
        self.bits[g] = row
        for w in diff:
            self.copy.touch(g * self.W + int(w))
        if diff.size:
            self.version[g] += 1
        else:
            self.ev["noop:set"] += 1

    def over(self, g, length):
        """the row as a predicate over the ids of the index: id < min(allow_bits, len)"""
        out = np.zeros(length, dtype=bool)
        k = min(length, self.allow_bits)
        out[:k] = self.bits[g, :k]
        return out

    def counted(self, g, del_version, length):
        """hnsw_mask_set::counted -> recounts (0 or 1); a recount ends the row's list"""
        if self.cache[g].use((self.version[g], del_version, length)):
            self.list_valid[g] = False
            return 1
        return 0

    def reserve(self, g, A, budget):
        """hnsw_mask_set::reserve_list: room for A ids within the budget; nothing is evicted"""
        if self.d_cap[g] and self.d_cap[g] >= A:
            return True
        cap = max(1, A)
        if self.list_bytes - self.d_cap[g] * 4 + cap * 4 > budget:
            return False
        self.list_bytes += (cap - self.d_cap[g]) * 4
        self.d_cap[g] = cap
        return True


def zero_delta():
    return {k: 0 for k in COUNTERS}


class Model:
    def __init__(self, d):
        self.ev = collections.Counter()
        self.d = d
        self.vecs = np.zeros((0, d), dtype=np.float32)
        self.levels = np.zeros(0, dtype=np.uint8)
        self.deleted = np.zeros(0, dtype=bool)
        self.labels = np.zeros(0, dtype=np.uint32)
        self.sets = {}
        self.exact_max, self.cache_mb = DEFAULT_EXACT_MAX, DEFAULT_CACHE_MB
        self.graph_version = 0
        self.seen_zero = False  # deleted_count went to 0 after having been above it
        self.after = None       # "clone" / "load": the next check is the first on the new handle
        self.inline_rows = -1
        self.step, self.first = -1, {}  # the step a noted event was first seen at (Machine.run sets `step`)
        self._new_handle(0, 0)

    def note(self, event):
        self.ev[event] += 1
        self.first.setdefault(event, self.step)

    @property
    def len(self):
        return self.vecs.shape[0]

    def _new_handle(self, del_nw, lab_nw):
        """the transport and cache state of a fresh handle whose host words were assigned (hnsw_clone, hnsw_load)"""
        self.del_copy, self.lab_copy = Copy("del", self.ev), Copy("lab", self.ev)
        self.del_nw, self.lab_nw = del_nw, lab_nw
        self.del_version, self.lab_version = 1, 1
        self.sort = Cache("sort", ("version", "del", "len"), self.ev)
        self.snap_valid = False
        self.patched = set()      # ids insert_vec patched into the live snapshot since the last whole upload
        self.lab_changed = set()  # ids whose label changed since the label column last went to HBM

    # ---- mutating ops ----
    def insert(self, vecs, levels):
        before = self.len
        self.vecs = np.concatenate([self.vecs, np.asarray(vecs, dtype=np.float32).reshape(-1, self.d)])
        self.levels = np.concatenate([self.levels, np.asarray(levels, dtype=np.uint8).reshape(-1)])
        grow = self.len - before
        self.deleted = np.concatenate([self.deleted, np.zeros(grow, dtype=bool)])
        self.labels = np.concatenate([self.labels, np.zeros(grow, dtype=np.uint32)])
        self.graph_version += 1
        for s in self.sets.values():
            if before <= s.allow_bits < self.len:
                self.ev["set:len_passes_allow_bits"] += 1

    def insert_vec(self, vecs, levels):
        """-> the point patches the inserts make (one each while the snapshot is live)"""
        before = self.len
        self.insert(vecs, levels)
        if self.snap_valid:
            self.patched.update(range(before, self.len))
        return len(levels) if self.snap_valid else 0

    def insert_bulk(self, vecs, levels):
        self.insert(vecs, levels)
        self.snap_valid = False

    def mark(self, ids, on):
        self.del_nw = max(self.del_nw, words_of(self.len))  # (the mask grows to cover the index, whatever changes)
        before, changed = int(self.deleted.sum()), False
        for i in ids:
            if bool(self.deleted[i]) != on:
                self.deleted[i] = on
                self.del_version += 1
                self.del_copy.touch(int(i) >> 6)
                changed = True
        after = int(self.deleted.sum())
        if not changed:
            self.ev["noop:del"] += 1
        if before > 0 and after == 0:
            self.seen_zero = True
            self.ev["del:to_zero"] += 1
        if before == 0 and after > 0 and self.seen_zero:
            self.ev["del:back_up"] += 1

    def set_labels(self, values, ids=None):
        self.lab_nw = max(self.lab_nw, (self.len + 1) // 2)
        ids = range(len(values)) if ids is None else ids
        changed = False
        for i, v in zip(ids, values):
            if int(self.labels[i]) != int(v):
                self.labels[i] = v
                self.lab_version += 1
                self.lab_copy.touch(int(i) >> 1)
                self.lab_changed.add(int(i))
                changed = True
        if not changed:
            self.ev["noop:lab"] += 1

    def set_create(self, name, bits):
        self.sets[name] = SetModel(bits, self.ev)

    def set_close(self, name):
        del self.sets[name]

    def option(self, key, value):
        if key == "filter_exact_max":
            self.exact_max = value
        elif key == "mask_set_cache_mb":
            self.cache_mb = value
        elif key == "inline_rows":
            self.inline_rows = value
            self.snap_valid = False  # (the snapshot is released and rebuilt by the next search)

    def clone(self):
        """the run continues on the clone: the host words and every option travel, the HBM copies, the caches and the
        sets do not (the sets are made again from the model)"""
        self._new_handle(self.del_nw, self.lab_nw)
        self._remake_sets()
        self.after = "clone"

    def save_load(self):
        """... on the loaded handle: the file `deleted` gives words for every id when an id is deleted, none otherwise;
        the options are the defaults"""
        self._new_handle(words_of(self.len) if self.deleted.any() else 0, 0)
        self.exact_max, self.cache_mb, self.inline_rows = DEFAULT_EXACT_MAX, DEFAULT_CACHE_MB, -1
        self._remake_sets()
        self.after = "load"

    def _remake_sets(self):
        self.sets = {name: SetModel(s.bits, self.ev) for name, s in self.sets.items()}

    # ---- what a call does to the copies and caches ----
    def ensure_uploaded(self):
        if self.snap_valid:
            return 0
        self.snap_valid = True
        self.patched.clear()
        return 1

    def sync_deleted(self):
        if not self.deleted.any():
            return 0
        return self.del_copy.sync(self.del_nw, self.del_nw // 8 + 16)

    def sync_labels(self):
        self.lab_nw = max(self.lab_nw, (self.len + 1) // 2)  # (the mirror covers every id of the index)
        self.lab_changed.clear()
        return self.lab_copy.sync(self.lab_nw, self.lab_nw // 8 + 16)

    def sort_for(self):
        self.sort.use((self.lab_version, self.del_version, self.len))

    def in_ranges(self, members):
        lab = self.labels[: self.len].astype(np.int64)
        out = np.zeros(self.len, dtype=bool)
        for lo, hi in members:
            out |= (lab >= lo) & (lab <= hi)
        return out

    def live(self):
        return ~self.deleted[: self.len]

    def plan(self, nq, setname=None, keys=None, ranges=None, masks=None, exact_max=None, exact_only=False,
             one_query=False):
        """a host-pointer filtered call (search_filtered, filter_host.cpp) restated: keys[i] the row of query i (NONE:
        no row; keys None: no rows at all), ranges[i] its list of (lo, hi) members (None: the call has no label ranges),
        masks the caller's rows when it brings them.  -> (admissible [nq, len] bools, paths [nq], counter deltas; the
        compactions as (at least, at most) when the call is `one_query` from several threads)"""
        L, live = self.len, self.live()
        exact_max = self.exact_max if exact_max is None else exact_max
        s = self.sets[setname] if setname is not None else None
        ranged_call = ranges is not None
        adms, paths, groups = [], [], {}
        for qi in range(nq):
            key = NONE if keys is None and masks is None and s is None else (0 if keys is None else int(keys[qi]))
            rl = tuple((int(a), int(b)) for a, b in ranges[qi]) if ranged_call else None
            adm = live.copy()
            if key != NONE and s is not None:
                adm &= s.over(key, L)
            elif key != NONE and masks is not None:
                row = np.zeros(L, dtype=bool)
                k = min(L, len(masks[key]))
                row[:k] = np.asarray(masks[key], dtype=bool)[:k]
                adm &= row
            if ranged_call:
                adm &= self.in_ranges(rl)
            A = int(adm.sum())
            exact = exact_only or A <= exact_max
            adms.append(adm)
            paths.append(1 if exact else 0)
            g = groups.setdefault((key, rl), [A, exact, 0])
            g[2] += 1
        d = zero_delta()
        info = {}
        for (key, rl), (A, exact, n_named) in groups.items():
            has_words = key != NONE and (s.W != 0 if s is not None else masks is not None)
            ranged = ranged_call and (s is None or (rl[0] != FULL and (key == NONE or s.W != 0)))
            info[key, rl] = (has_words, ranged)
            if ranged:
                self.sort_for()
            if s is not None and has_words and not (ranged and rl[0][0] > rl[0][1]):
                d["mask_set_recounts"] += s.counted(key, self.del_version, L)
        d["uploads"] = self.ensure_uploaded()
        d["deleted_mask_words_uploaded"] = self.sync_deleted()
        if s is not None:
            d["mask_set_words_uploaded"] = s.copy.sync(s.G * s.W, 0)
        if ranged_call:
            d["label_words_uploaded"] = self.sync_labels()
        budget = (self.cache_mb << 20) if self.cache_mb > 0 else 0
        n_exact_groups = sum(1 for g in groups.values() if g[1])
        grouping = one_query and len(groups) > 1 and n_exact_groups > 1
        lo = hi = 0
        for (key, rl), (A, exact, n_named) in groups.items():
            has_words, ranged = info[key, rl]
            if s is None or not has_words or ranged or not exact or s.list_valid[key]:
                continue
            if s.reserve(key, A, budget):  # compacted into the set once, for this call and the ones after it
                s.list_valid[key] = True
                lo, hi = lo + 1, hi + 1
            elif one_query and nq > 1:     # beyond the budget: per call, and the calls of the threads are gathered freely
                lo, hi = lo + (1 if A > 0 else 0), hi + n_named
            else:
                lo, hi = lo + (0 if grouping and A == 0 else 1), hi + (0 if grouping and A == 0 else 1)
        d["mask_set_compactions"] = lo if lo == hi else (lo, hi)
        return adms, paths, d

    def device_call(self, setname, ranged):
        """a device-pointer filtered call: the copies are brought up to date, nothing is planned"""
        d = zero_delta()
        d["uploads"] = self.ensure_uploaded()
        d["deleted_mask_words_uploaded"] = self.sync_deleted()
        if ranged:
            d["label_words_uploaded"] = self.sync_labels()
        if setname is not None:
            s = self.sets[setname]
            d["mask_set_words_uploaded"] = s.copy.sync(s.G * s.W, 0)
        return d

    def count_labels(self, members):
        """hnsw_count_labels_in_ranges: the planner's count, over its sorted copy"""
        self.sort_for()
        return int((self.in_ranges(members) & self.live()).sum())

    def dist64(self, q, cosine=False):
        """the distances of a vector to every row, in float64 from the model's own vectors (under the cosine option:
        between the unit vectors)"""
        rows, q = self.vecs.astype(np.float64), np.asarray(q, dtype=np.float64)
        if cosine:
            rows = rows / np.maximum(np.linalg.norm(rows, axis=1), 1e-300)[:, None]
            q = q / max(np.linalg.norm(q), 1e-300)
        return np.sqrt(((rows - q[None, :]) ** 2).sum(axis=1))

    def nearest(self, q, k, adm=None, cosine=False):
        """the k nearest admissible (None: live) ids of a vector by dist64, ascending"""
        adm = self.live() if adm is None else adm
        ids = np.flatnonzero(adm)
        d = self.dist64(q, cosine)[ids]
        return ids[np.argsort(d, kind="stable")[:k]]


# ---- the schedule -----------------------------------------------------------------------------------------------
def draw_vectors(rng, n, d, cosine):
    v = rng.random((n, d), dtype=np.float32)
    return v - np.float32(0.5) if cosine else v


def draw_levels(rng, n):
    return np.minimum((-np.log(1.0 - rng.random(n)) / np.log(M)).astype(np.int64), 3).astype(np.uint8)


def draw_range(rng):
    k = rng.random()
    if k < 0.2:
        return FULL
    if k < 0.3:
        return (5, 2)  # empty
    if k < 0.36:
        return (MAX, MAX)
    a, b = sorted(int(x) for x in rng.integers(0, 8, 2))
    return (a, b)


def draw_queries(rng, m, nq, cosine):
    """some fresh, some stored rows, some rows inserted during the run"""
    qs = []
    for _ in range(nq):
        k = rng.random()
        if k < 0.4 or m.len == 0:
            qs.append(draw_vectors(rng, 1, m.d, cosine)[0])
        elif k < 0.7 or m.len <= N0:
            qs.append(m.vecs[int(rng.integers(min(m.len, N0)))])
        else:
            qs.append(m.vecs[int(rng.integers(N0, m.len))])
    return np.stack(qs).astype(np.float32)


def draw_check(rng, m, cosine, family=None, used=None, hint=None):
    """the check after an op.  `used` (family -> draws so far) keeps the families in balance: the least drawn of those
    the state allows is next, ties broken by the draw; and a family's draws take turns at filter_exact_max"""
    used = collections.Counter() if used is None else used
    fams = ["search_batch", "filtered", "multi", "range", "ranges", "range_device", "one", "one_threads", "grouped",
            "grouped_range", "brute_force", "count_labels", "deleted_ids", "get_labels"]
    if m.sets:
        fams += ["set", "set_range", "set_device", "set_range_device", "grouped_row", "set_count_read"]
    if family is None:
        least = min(used[f] for f in fams)
        fams = [f for f in fams if used[f] == least]
        family = fams[int(rng.integers(len(fams)))]
    turn = used[family]
    used[family] += 1
    c = {"family": family}
    if family in HOST_FAMILIES:
        if family == "count_labels":
            c["members"] = [draw_range(rng) for _ in range(int(rng.integers(0, 4)))]
        return c
    nq = 8 if family == "one_threads" else 1 if family == "one" else int(rng.integers(3, 6))
    c["Q"] = draw_queries(rng, m, nq, cosine)
    c["n"] = int(rng.choice([1, 7, 10, 33]))
    c["ef"] = int(rng.choice([8, 32, 64, 200]))
    live = int(m.live().sum())
    c["exact_max"] = (-1, HUGE, int(rng.integers(10, max(11, live // 2))), -1)[turn % 4]
    L = m.len
    if family == "filtered":
        bits = int(rng.choice([L, max(1, L - int(rng.integers(1, 70))), L + int(rng.integers(1, 70))]))
        c["masks"] = [rng.random(bits) < rng.choice([0.5, 0.1, 0.02])]
    if family == "multi":
        c["masks"] = [rng.random(L) < f for f in (0.5, 0.08, 0.0)]
        c["keys"] = [int(x) for x in rng.choice([0, 1, 2, NONE], nq)]
    if family in ("set", "set_range", "set_device", "set_range_device", "grouped_row") or \
            (family in ("one", "one_threads") and m.sets and rng.random() < 0.7):
        name = hint[0] if hint else sorted(m.sets)[int(rng.integers(len(m.sets)))]
        c["set"] = name
        c["keys"] = [int(x) for x in rng.choice(list(range(m.sets[name].G)) + [NONE], nq)]
        if hint:
            c["keys"][0] = hint[1]  # (the row the op was about is named)
    if family in ("range", "range_device", "set_range", "set_range_device", "grouped_range", "one", "one_threads") or \
            (family == "grouped_row" and rng.random() < 0.3):
        c["ranges"] = [[draw_range(rng)] for _ in range(nq)]
    if family == "ranges":
        c["ranges"] = [[draw_range(rng) for _ in range(int(rng.integers(0, 4)))] for _ in range(nq)]
    if family.startswith("grouped"):
        c["pool"] = int(rng.choice([8, 24, 64]))
        c["G"] = int(rng.integers(1, min(c["pool"], 6) + 1))
        c["P"] = int(rng.integers(1, min(c["pool"], 4) + 1))
    if family == "brute_force":
        c["n"] = int(rng.choice([1, 10, 32]))
    return c


def draw_set_bits(rng, L, allow_bits):
    G = int(rng.integers(3, 5))  # (at least 9 words from 129 bits on: one changed word is scattered, two are a whole copy)
    bits = np.zeros((G, allow_bits), dtype=bool)
    for g in range(G):
        bits[g] = rng.random(allow_bits) < rng.choice([0.5, 0.15, 0.03])
    return bits


def draw_multi_vectors(rng, m, cosine, nq, T, recent):
    """[nq, T, d]: draw_queries per query; sometimes one vector twice in a query (its two lists hold the same ids),
    sometimes a stored row as a vector (often one that insert_vec appended lately)"""
    Q = np.stack([draw_queries(rng, m, T, cosine) for _ in range(nq)])
    for q in range(nq):
        if T > 1 and rng.random() < 0.4:
            Q[q, 1] = Q[q, 0]
        if rng.random() < 0.5:
            i = recent[int(rng.integers(len(recent)))] if recent and rng.random() < 0.7 else int(rng.integers(m.len))
            Q[q, T - 1] = m.vecs[i]
    return np.ascontiguousarray(Q, dtype=np.float32)


def draw_sources(rng, m, nq, width, recent):
    """[nq, width] source ids: old rows, rows inserted during the run (often one that insert_vec appended lately), the id
    len - 1 and absent slots; no query with every slot absent"""
    src = np.full((nq, width), MAX, dtype=np.uint32)
    for q in range(nq):
        for s in range(width):
            k = rng.random()
            if k < 0.15:
                continue
            if k < 0.4:
                src[q, s] = int(rng.integers(min(m.len, N0)))
            elif k < 0.75 and recent:
                src[q, s] = recent[int(rng.integers(len(recent)))]
            elif k < 0.85:
                src[q, s] = m.len - 1
            else:
                src[q, s] = int(rng.integers(m.len))
        if (src[q] == MAX).all():
            src[q, int(rng.integers(width))] = m.len - 1
    return src


def draw_radii(rng, m, cosine, c, turn):
    """the radii of a radius check, from the model alone (Model.dist64): a scalar that no row lies within (the queries
    are then fresh vectors, none of them a stored row), per query twice the distance of its j-th nearest live row (the
    nearest few lie within whatever f32 or the 8-bit codes round), +inf, or one of the three per query"""
    nq = c["Q"].shape[0]
    kind = ("none", "few", "inf", "mixed")[turn % 4]
    if kind == "none":
        c["Q"] = draw_vectors(rng, nq, m.d, cosine)
    live = m.live()
    near = [np.sort(m.dist64(q, cosine)[live])[:4] for q in c["Q"]]
    if kind == "none":
        c["radius"] = float(np.float32(0.5 * min(d[0] for d in near)))
    elif kind == "inf":
        c["radius"] = float("inf")
    else:
        r = np.zeros(nq, dtype=np.float32)
        for q in range(nq):
            k = "few" if kind == "few" else ("none", "few", "inf")[int(rng.integers(3))]
            j = int(rng.choice([1, 2, 4]))
            r[q] = np.inf if k == "inf" else 0.5 * near[q][0] if k == "none" else 2.0 * near[q][min(j, len(near[q])) - 1]
        c["radius"] = r
    c["radius_kind"] = kind


def draw_composite_check(rng, m, cosine, used, recent, hint=None, family=None, anchors=True):
    """the check after an op of a composite schedule: one of COMPOSITE_FAMILIES or an anchor, the least drawn (in the
    state: ids deleted or none) first.  While the call takes the host form -- ids are deleted, or the family brings a
    filter -- a family's draws take turns: filter_exact_max -1 (the graph path), beyond every count (the exact path), a
    REFUSED call at the host form's limit + 1, a drawn filter_exact_max"""
    deleted = bool(m.deleted.any())
    state = "del" if deleted else "nodel"
    fams = list(COMPOSITE_FAMILIES) + (list(ANCHORS) if anchors else [])
    if not m.sets:
        fams.remove("diverse_row")
    if family is None:
        least = min(used[f, state] for f in fams)
        fams = [f for f in fams if used[f, state] == least]
        family = fams[int(rng.integers(len(fams)))]
    used[family, state] += 1
    if family in ANCHORS:
        return draw_check(rng, m, cosine, family, used["anchors"])
    host_form = deleted or family in FILTERED_COMPOSITES
    turn = used[family, "turn", host_form]
    used[family, "turn", host_form] += 1
    c = {"family": family}
    live = int(m.live().sum())
    c["ef"] = int(rng.choice([8, 32, 64, 200]))
    c["exact_max"] = (-1, HUGE, -1, int(rng.integers(10, max(11, live // 2))))[turn % 4] if host_form else -1
    refused = host_form and turn % 4 == 2
    if refused:
        c["refused"] = True
    pool = REFUSED_POOL if refused else int(rng.choice(HOST_POOLS if host_form else DEVICE_POOLS))
    if family in ("multi_vec", "late"):
        nq = int(rng.integers(2, 4))
        T = int(rng.choice([1, 2, 3] if refused else [1, 2, 3, 5]))
        limit = FUSE_MAX_CANDS if family == "multi_vec" else LATE_MAX_CANDS
        if not refused:
            pool = int(rng.choice([p for p in (HOST_POOLS if host_form else DEVICE_POOLS) if T * p <= limit]))
        c["Q"] = draw_multi_vectors(rng, m, cosine, nq, T, recent)
        c["mode"] = int(rng.integers(2))
        c["n"] = int(rng.integers(1, min(pool, 10) + 1))
        if family == "multi_vec" and rng.random() < 0.6:
            c["weights"] = (rng.random((nq, T), dtype=np.float32) * np.float32(2.0) + np.float32(0.25)).astype(np.float32)
    elif family in ("from_rows", "by_id"):
        nq = int(rng.integers(3, 6))
        width = 1 if family == "by_id" else int(rng.choice([1, 3, 8]))
        c["src"] = draw_sources(rng, m, nq, width, recent)
        c["n"] = max(pool - width, 1)  # (the call's limit is on n + width)
        c["exclude"] = bool(rng.random() < 0.5)
        if family == "from_rows" and rng.random() < 0.6:
            c["weights"] = ((rng.random((nq, width), dtype=np.float32) - np.float32(0.25)) * np.float32(2.0)).astype(np.float32)
        if refused:
            c["n"] = REFUSED_POOL - width
    else:
        nq = int(rng.integers(3, 6))
        c["Q"] = draw_queries(rng, m, nq, cosine)
    c["pool"] = pool
    if family == "radius":
        c["n_first"] = int(rng.choice([f for f in (1, 4, 16) if f <= pool]))
        draw_radii(rng, m, cosine, c, turn)
    if family.startswith("diverse"):
        c["n"] = int(rng.integers(1, min(pool, 10) + 1))
        c["lam"] = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
    if family == "diverse_row":
        name = hint[0] if hint and hint[0] in m.sets else sorted(m.sets)[int(rng.integers(len(m.sets)))]
        c["set"] = name
        c["keys"] = [int(x) for x in rng.choice(list(range(m.sets[name].G)) + [NONE], nq)]
    if family == "diverse_range" or (family == "diverse_row" and rng.random() < 0.3):
        c["ranges"] = [[draw_range(rng)] for _ in range(nq)]
    return c


def schedule(seed, kind, steps=None, cosine=False, families="default"):
    """-> the ops of a run, each {"op": ..., its arguments, "check": the check that follows it}.  (`kind` does not change
    the draws: both vector kinds run the same ops.)  families "default": the committed schedules (SEEDS, STEPS), whose
    draws tests/test_update_machine_host.py pins by a digest.  "composite": the same ops, weights and forced events, the
    checks drawn by draw_composite_check, and two more forced events: every id unmarked and then QUIET ops that mark
    nothing (the composite calls take their device form on a handle that has held deletions), with inline_rows set to 1
    between two composite checks of that stretch; and the check after the clone and after the save / load is one of
    every family, the anchors included, in turn ("more")."""
    composite = families == "composite"
    assert composite or families == "default", families
    steps = (COMPOSITE_STEPS if composite else STEPS) if steps is None else steps
    rng = np.random.default_rng([int(seed), 0x5EED])
    m = Model(D)
    ops = []

    used = collections.Counter()
    if composite:
        used = collections.defaultdict(int)
        used["anchors"] = collections.Counter()
    recent = []  # (composite) the ids insert_vec appended since the snapshot was last made whole

    def emit(op, family=None, hint=None):
        apply_op(m, op)
        if not composite:
            op["check"] = draw_check(rng, m, cosine, family, used, hint)
        else:
            o = op["op"]
            if o == "insert_vec":
                recent.extend(range(m.len - len(op["levels"]), m.len))
            elif o in ("insert_bulk", "clone", "save_load") or (o == "option" and op["key"] == "inline_rows"):
                del recent[:]
            if o in ("clone", "save_load"):
                fams = [f for f in COMPOSITE_FAMILIES + ANCHORS if m.sets or f != "diverse_row"]
                k = (int(seed) + (o == "save_load")) % len(fams)
                cs = [draw_composite_check(rng, m, cosine, used, recent, family=f) for f in fams[k:] + fams[:k]]
                op["check"] = dict(cs[0], more=cs[1:])
            else:
                op["check"] = draw_composite_check(rng, m, cosine, used, recent, hint, anchors=not quiet["composite_only"])
        ops.append(op)

    QUIET = 17  # ops after the unmark of everything that mark nothing
    quiet = {"start": None, "flipped": False, "inserts": 0, "composite_only": False}

    emit({"op": "insert_bulk", "vecs": draw_vectors(rng, N0, D, cosine), "levels": draw_levels(rng, N0)})
    emit({"op": "set_create", "name": "A", "bits": draw_set_bits(rng, m.len, m.len + 24)})  # above len: passed by inserts
    emit({"op": "set_labels", "ids": None, "values": rng.integers(0, 8, m.len).astype(np.uint32)}, "range")
    emit({"op": "mark", "ids": rng.choice(m.len, 3, replace=False)}, "search_batch")
    forced = [(int(steps * 0.15), "grow_within"), (int(steps * 0.30), "top_layer"), (int(steps * 0.45), "insert_bulk"), (int(steps * 0.62), "clone"),
              (int(steps * 0.80), "save_load")]
    weights = {"insert_vec": 20, "mark_few": 9, "mark_many": 3, "mark_again": 3, "unmark": 6, "unmark_all": 2,
               "labels_some": 8, "labels_all": 2, "labels_same": 3, "labels_new": 4, "set_create": 3, "set_update": 10,
               "set_update_same": 3, "set_write": 4, "set_close": 2, "exact_max": 3, "inline_rows": 2, "cache_mb": 3}
    names, p = list(weights), np.array(list(weights.values()), dtype=np.float64)
    p /= p.sum()
    last_labelled = N0
    if composite:
        forced.insert(3, (int(steps * 0.47), "quiet"))
    while len(ops) < steps:
        in_quiet = quiet["start"] is not None and len(ops) - quiet["start"] < QUIET
        if in_quiet:
            # nothing is marked; after five ops inline_rows is set to 1 between two composite checks, and two inserts follow
            # it, patched into the snapshot that the check after the flip made
            pos = len(ops) - quiet["start"]
            quiet["composite_only"] = pos >= 2 and not quiet["flipped"]  # (an op may bring two checks: from 2 on)
            if pos >= 5 and not quiet["flipped"]:
                what = "inline_on"
            elif quiet["flipped"] and quiet["inserts"] < 2:
                what = "insert_vec"
                quiet["inserts"] += 1
            else:
                what = names[int(rng.choice(len(names), p=p))]
                if "mark" in what or what == "inline_rows":
                    continue
        else:
            quiet["composite_only"] = False
            what = forced.pop(0)[1] if forced and len(ops) >= forced[0][0] else names[int(rng.choice(len(names), p=p))]
        L = m.len
        dele = np.flatnonzero(m.deleted)
        if what.startswith("mark") and dele.size > L // 4:
            continue  # (most ids stay live)
        if composite and what in ("clone", "save_load") and not m.sets:  # (diverse_row is among the checks that follow)
            emit({"op": "set_create", "name": "A", "bits": draw_set_bits(rng, L, L + 24)})
        if what == "quiet":
            if dele.size:
                emit({"op": "unmark", "ids": dele})
            quiet["start"] = len(ops)
        elif what == "inline_on":
            emit({"op": "option", "key": "inline_rows", "value": 1})
            quiet["flipped"] = True
        elif what == "insert_vec":
            k = int(rng.integers(1, 9))
            emit({"op": "insert_vec", "vecs": draw_vectors(rng, k, D, cosine), "levels": draw_levels(rng, k)})
        elif what == "grow_within":
            # the deleted mask's host words grow by one within the copy's capacity with no word listed: a mark whose
            # mask goes to HBM, inserts up to the next word of 64 ids, a mark of ids already deleted
            emit({"op": "mark", "ids": rng.choice(L, 2, replace=False)}, "search_batch")
            k = 64 - L % 64 + 1
            emit({"op": "insert_vec", "vecs": draw_vectors(rng, k, D, cosine), "levels": draw_levels(rng, k)})
            emit({"op": "mark", "ids": np.flatnonzero(m.deleted)[:2]}, "search_batch")
            # ... and by one more with a word listed: a mark of a new id
            emit({"op": "insert_vec", "vecs": draw_vectors(rng, 64, D, cosine), "levels": draw_levels(rng, 64)})
            emit({"op": "mark", "ids": np.array([m.len - 1])}, "search_batch")
        elif what == "top_layer":
            emit({"op": "insert_vec", "vecs": draw_vectors(rng, 1, D, cosine),
                  "levels": np.array([int(m.levels.max()) + 1], dtype=np.uint8)})
        elif what == "insert_bulk":
            # a mark whose mask goes to HBM, then enough points to outgrow that copy's capacity whenever it was made, then
            # a mark of ids already deleted: the host words grow to the index length and no word is listed
            emit({"op": "mark", "ids": rng.choice(L, 2, replace=False)}, "search_batch")
            cap_ids = 64 * (words_of(L) + words_of(L) // 8 + 16)
            k = cap_ids + 70 - L
            emit({"op": "insert_bulk", "vecs": draw_vectors(rng, k, D, cosine), "levels": draw_levels(rng, k)})
            emit({"op": "mark", "ids": np.flatnonzero(m.deleted)[:2]}, "search_batch")
        elif what == "mark_few":
            emit({"op": "mark", "ids": rng.choice(L, int(rng.integers(1, 4)), replace=False)})
        elif what == "mark_many":  # ids in more than an eighth of the words
            nw = words_of(L)
            ws = rng.choice(nw, min(nw, nw // 8 + 2), replace=False)
            ids = np.unique(np.minimum(ws * 64 + rng.integers(0, 64, ws.size), L - 1))
            emit({"op": "mark", "ids": ids})
        elif what == "mark_again":
            if dele.size == 0:
                continue
            emit({"op": "mark", "ids": rng.choice(dele, min(dele.size, 2), replace=False)})
        elif what == "unmark":
            if dele.size == 0:
                continue
            ids = rng.choice(dele, min(dele.size, int(rng.integers(1, 4))), replace=False)
            if rng.random() < 0.3:
                ids = np.concatenate([ids, rng.choice(L, 1)])  # (one that may not be deleted)
            emit({"op": "unmark", "ids": ids})
        elif what == "unmark_all":
            if dele.size == 0:
                continue
            emit({"op": "unmark", "ids": dele})
            emit({"op": "mark", "ids": rng.choice(L, 2, replace=False)})  # ... followed by a new mark
        elif what == "labels_some":
            ids = rng.choice(L, int(rng.integers(1, 12)), replace=False)
            vals = rng.integers(0, 8, ids.size).astype(np.uint32)
            if rng.random() < 0.15:
                vals[0] = MAX
            emit({"op": "set_labels", "ids": ids, "values": vals})
        elif what == "labels_all":
            emit({"op": "set_labels", "ids": None, "values": rng.integers(0, 8, L).astype(np.uint32)})
            last_labelled = L
        elif what == "labels_same":
            ids = rng.choice(L, 3, replace=False)
            emit({"op": "set_labels", "ids": ids, "values": m.labels[ids].copy()})
        elif what == "labels_new":
            if last_labelled >= L:
                continue
            ids = np.arange(last_labelled, L)
            emit({"op": "set_labels", "ids": ids, "values": rng.integers(1, 8, ids.size).astype(np.uint32)})
            last_labelled = L
        elif what == "set_create":
            name = "A" if "A" not in m.sets else "B" if "B" not in m.sets else None
            if name is None:
                continue
            bits = int(rng.choice([L, max(1, L - int(rng.integers(1, 40))), L + int(rng.integers(1, 40))]))
            emit({"op": "set_create", "name": name, "bits": draw_set_bits(rng, L, bits)})
        elif what in ("set_update", "set_update_same", "set_write", "set_close"):
            if not m.sets:
                continue
            name = sorted(m.sets)[int(rng.integers(len(m.sets)))]
            s = m.sets[name]
            g = int(rng.integers(s.G))
            if what == "set_update":
                allow = bool(rng.random() < 0.6)
                ids = rng.choice(s.allow_bits, int(rng.choice([1, 2, 30])), replace=False)
                # (often between two searches that name the row: the words of one update travel alone, and of the
                # row's three keys only its version moves)
                fams = ["set", "set_range", "grouped_row"]
                if rng.random() < 0.6:
                    on = np.flatnonzero(s.bits[g])[:1]
                    emit({"op": "set_update", "name": name, "row": g, "ids": on, "allow": True},
                         str(rng.choice(fams)), (name, g))
                    emit({"op": "set_update", "name": name, "row": g, "ids": ids, "allow": allow},
                         str(rng.choice(fams + ["set_device"])), (name, g))
                else:
                    emit({"op": "set_update", "name": name, "row": g, "ids": ids, "allow": allow})
            elif what == "set_update_same":
                on = np.flatnonzero(s.bits[g])
                if on.size == 0:
                    continue
                emit({"op": "set_update", "name": name, "row": g, "ids": on[:2], "allow": True})
            elif what == "set_write":
                row = s.bits[g].copy() if rng.random() < 0.2 else rng.random(s.allow_bits) < rng.choice([0.4, 0.05])
                emit({"op": "set_write", "name": name, "row": g, "bits": row})
            elif len(m.sets) > 1 or rng.random() < 0.5:
                emit({"op": "set_close", "name": name})
        elif what == "exact_max":
            emit({"op": "option", "key": "filter_exact_max", "value": int(rng.choice([-1, 40, 1 << 40]))})
        elif what == "inline_rows":
            emit({"op": "option", "key": "inline_rows", "value": int(rng.choice([-1, 0, 1]))})
        elif what == "cache_mb":
            emit({"op": "option", "key": "mask_set_cache_mb", "value": int(rng.choice([0, 0, DEFAULT_CACHE_MB]))})
        elif what == "clone":
            # the clone is mutated once first (and the parent's host-visible state must not move)
            emit({"op": "clone", "first": {"mark": rng.choice(L, 2, replace=False),
                                           "labels": (rng.choice(L, 2, replace=False), np.array([9, 9], dtype=np.uint32))}})
        elif what == "save_load":
            emit({"op": "save_load"})
    return ops[:steps]


def apply_op(m, op):
    """one op on the model -> the point patches it predicts"""
    o = op["op"]
    if o == "insert_vec":
        return m.insert_vec(op["vecs"], op["levels"])
    if o == "insert_bulk":
        m.insert_bulk(op["vecs"], op["levels"])
    elif o in ("mark", "unmark"):
        m.mark(op["ids"], o == "mark")
    elif o == "set_labels":
        m.set_labels(op["values"], op["ids"])
    elif o == "set_create":
        m.set_create(op["name"], op["bits"])
    elif o == "set_update":
        m.sets[op["name"]].update(op["row"], op["ids"], op["allow"])
    elif o == "set_write":
        m.sets[op["name"]].write(op["row"], op["bits"])
    elif o == "set_close":
        m.set_close(op["name"])
    elif o == "option":
        m.option(op["key"], op["value"])
    elif o == "clone":
        m.clone()
        m.mark(op["first"]["mark"], True)
        m.set_labels(op["first"]["labels"][1], op["first"]["labels"][0])
    elif o == "save_load":
        m.save_load()
    else:
        raise ValueError(o)
    return 0


def describe(op):
    """an op in one line, for a failure's message"""
    out = []
    for k, v in op.items():
        if k == "check":
            continue
        if isinstance(v, np.ndarray):
            v = v.tolist() if v.size <= 8 else "%s%s" % (v.dtype, list(v.shape))
        out.append("%s=%s" % (k, v))
    return " ".join(out)


def _canon(v, h):
    if isinstance(v, dict):
        h.update(b"{")
        for k in sorted(v):
            h.update(str(k).encode())
            _canon(v[k], h)
        h.update(b"}")
    elif isinstance(v, np.ndarray):
        h.update(("%s%s" % (v.dtype.str, list(v.shape))).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)):
        h.update(b"[")
        for x in v:
            _canon(x, h)
        h.update(b"]")
    else:
        h.update(repr(v.item() if isinstance(v, np.generic) else v).encode())


def digest(ops):
    """sha256 over describe(op), the check (every key, arrays by their bytes) and the query bytes of every op of a schedule"""
    h = hashlib.sha256()
    for op in ops:
        h.update(describe(op).encode())
        _canon(op["check"], h)
        h.update(np.ascontiguousarray(op["check"].get("Q", np.zeros(0, dtype=np.float32))).tobytes())
    return h.hexdigest()


# ---- the machine ------------------------------------------------------------------------------------------------
def unit(x):
    """rows / their norm, the sum of squares taken in order in float32 (as the library normalises under cosine)"""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros(x.shape[0], dtype=np.float32)
    for e in range(x.shape[1]):
        s = s + x[:, e] * x[:, e]
    return x / np.sqrt(s)[:, None]


class Machine:
    def __init__(self, seed, kind, product=None, steps=None, cosine=False, families="default"):
        self.seed, self.kind, self.product, self.cosine = seed, kind, product, cosine
        self.ops = schedule(seed, kind, steps, cosine, families)
        self.n_expected = sum(1 + len(op["check"].get("more", ())) for op in self.ops)
        # what the composite restatements read of the model, changed on purpose by the sensitivity tests alone
        # (tests/test_gpu_update_machine.py): id -> label, id -> (component, ulps)
        self.tamper_labels, self.tamper_rows = {}, {}
        self.m = Model(D)
        self.index, self.sets = None, {}
        self.step, self.family, self.qi = -1, None, None
        self.n_checks = 0
        self._rows = None        # the restatement's rows (dequantised once per point)
        self._ridx_for = self._orc_for = None
        self.tmp = None

    # ---- driving ----
    def run(self, upto=None):
        try:
            for self.step, op in enumerate(self.ops[: upto]):
                self.family, self.qi = None, None
                self.m.step = self.step
                try:
                    self.apply(op)
                    self.check_host_state()
                    after = self.m.after
                    for c in [op["check"]] + list(op["check"].get("more", ())):
                        self.family, self.qi = c["family"], None
                        if after:
                            self.m.note("check_after:%s:%s" % (after, self.family))
                        self.check(c)
                except AssertionError as e:
                    raise AssertionError("seed %d kind %d step %d op [%s] check family %s query %s: %s" % (
                        self.seed, self.kind, self.step, describe(op), self.family, self.qi, e)) from e
        finally:
            self.close()
        return self

    def close(self):
        for s in self.sets.values():
            s.close()
        self.sets = {}
        self.index = None
        if self.tmp:
            shutil.rmtree(self.tmp, ignore_errors=True)
            self.tmp = None

    def stats(self):
        return {k: self.index.stat(k) for k in COUNTERS}

    def expect_delta(self, before, want, what):
        got = {k: self.index.stat(k) - v for k, v in before.items()}
        for k in COUNTERS:
            w = want[k]
            lo, hi = w if isinstance(w, tuple) else (w, w)
            assert lo <= got[k] <= hi, "%s: counter %s moved by %d, the model says %s (all: %s)" % (what, k, got[k], w, got)

    # ---- ops ----
    def apply(self, op):
        import hnsw_rs_amd as H
        o = op["op"]
        if self.product is None:
            apply_op(self.m, op)
            return
        before = self.stats() if self.index is not None and self.product == "gpu" else None
        if self.index is None:
            self.index = H.HNSW.new(M, EF_CONS, D, self.kind)
            if self.cosine:
                self.index.set_option("metric_cosine", 1)
        patches = 0
        if o == "insert_vec":
            for v, lv in zip(op["vecs"], op["levels"]):
                got = self.index.insert_vec(v, level=int(lv))
                assert got == self.m.len, "insert_vec returned id %d at length %d" % (got, self.m.len)
                patches += apply_op(self.m, {"op": "insert_vec", "vecs": v[None], "levels": [lv]})
        else:
            apply_op(self.m, op)
        if o == "insert_bulk":
            self.index.insert_bulk(op["vecs"], 1, False, levels=op["levels"])
        elif o == "mark":
            self.index.mark_deleted(op["ids"])
        elif o == "unmark":
            self.index.unmark_deleted(op["ids"])
        elif o == "set_labels":
            self.index.set_labels(op["values"], op["ids"])
        elif o == "set_create":
            self.sets[op["name"]] = self.index.mask_set(op["bits"])
        elif o == "set_update":
            self.sets[op["name"]].update(op["row"], op["ids"], op["allow"])
        elif o == "set_write":
            self.sets[op["name"]].write(op["row"], op["bits"])
        elif o == "set_close":
            self.sets.pop(op["name"]).close()
        elif o == "option":
            self.index.set_option(op["key"], op["value"])
        elif o == "clone":
            self.clone(op)
            before = None
        elif o == "save_load":
            self.save_load()
            before = None
        assert self.index.len() == self.m.len
        if before is not None:
            want = zero_delta()
            want["point_patches"] = patches
            self.expect_delta(before, want, "the op itself")

    def host_state(self, index):
        return (index.len(), index.deleted_count(), index.deleted_ids().tolist(), index.get_labels().tolist())

    def remake_sets(self):
        for s in self.sets.values():
            s.close()
        self.sets = {name: self.index.mask_set(s.bits) for name, s in self.m.sets.items()}

    def clone(self, op):
        parent = self.index
        was = self.host_state(parent)
        for s in self.sets.values():
            s.close()
        self.sets = {}
        self.index = parent.clone()
        assert self.host_state(self.index) == was, "the clone does not start with its parent's host state"
        self.index.mark_deleted(op["first"]["mark"])
        self.index.set_labels(op["first"]["labels"][1], op["first"]["labels"][0])
        assert self.host_state(parent) == was, "a change of the clone moved its parent"
        del parent
        self.remake_sets()

    def save_load(self):
        import hnsw_rs_amd as H
        was = self.host_state(self.index)
        self.tmp = self.tmp or tempfile.mkdtemp(prefix="update_machine_")
        path = os.path.join(self.tmp, "step%d" % self.step)
        self.index.save(path)
        for s in self.sets.values():
            s.close()
        self.sets = {}
        self.index = H.HNSW.load(path)
        if self.cosine:
            self.index.set_option("metric_cosine", 1)  # (the file format has no field for a metric)
        assert self.host_state(self.index) == was, "the loaded handle does not hold what was saved"
        self.remake_sets()

    # ---- the host-visible state, after every op ----
    def check_host_state(self):
        if self.product is None:
            return
        import hnsw_rs_amd as H
        m, index = self.m, self.index
        dele = np.flatnonzero(m.deleted)
        assert index.deleted_count() == dele.size, "deleted_count %d, the model %d" % (index.deleted_count(), dele.size)
        assert np.array_equal(index.deleted_ids(), dele), "deleted_ids differ from the model"
        for i in {0, m.len - 1, m.len // 2} | set(dele[:3].tolist()):
            assert index.is_deleted(i) == bool(m.deleted[i]), "is_deleted(%d)" % i
        assert np.array_equal(index.get_labels(), m.labels), "get_labels differs from the model"
        assert sorted(self.sets) == sorted(m.sets)
        for name, s in self.sets.items():
            ms = m.sets[name]
            assert (s.n_masks, s.allow_bits) == (ms.G, ms.allow_bits)
            for g in range(ms.G):
                assert np.array_equal(s.read(g), H.pack_allow(ms.bits[g])[0][: ms.W]), "set %s row %d: read" % (name, g)
                assert s.count(g) == int(ms.bits[g].sum()), "set %s row %d: count" % (name, g)

    # ---- the restatements over the product's graph ----
    def rvecs(self):
        return unit(self.m.vecs) if self.cosine else self.m.vecs

    def ridx(self):
        from oracle import restate_np as R
        if self._ridx_for != (id(self.index), self.m.graph_version):
            index, vs = self.index, self.rvecs()
            done = 0 if self._rows is None else self._rows.shape[0]
            layers = [index.get_layer(l).csr() for l in range(index.nb_layers())]
            r = R.Index.from_csr(vs[done:], index.vec_kind, layers, int(index.params.ep))  # (tests.test_gpu_filtered.restated)
            self._rows = r.rows if self._rows is None else np.concatenate([self._rows, r.rows])
            r.rows = self._rows
            self._ridx, self._ridx_for = r, (id(self.index), self.m.graph_version)
        return self._ridx

    def orc(self):
        from tests.util import oracle_from_product
        if self._orc_for != (id(self.index), self.m.graph_version):
            self._orc = oracle_from_product(self.index, self.rvecs(), self.m.levels)
            self._orc_for = (id(self.index), self.m.graph_version)
        return self._orc

    def want(self, q, n, ef, adm, path):
        from tests import filtered_restate as FR
        from tests.test_gpu_filtered import LIMIT
        if path == 1:
            return FR.exact(self.ridx(), q, n, np.flatnonzero(adm))
        a = adm.tolist()
        g = FR.graph(self.ridx(), q, n, ef, lambda i: a[i])
        assert g["visited0"] + g["maxdeg0"] <= LIMIT, "the shapes were to stay far below the visited limit"
        return g

    def compare(self, got, Q, n, ef, adms, paths, what):
        """ids, distance bits, counts, (n_dist, n_exp, sum_deg), status and path of every query"""
        from tests.test_gpu_filtered_multi import compare_row
        Qr = unit(Q) if self.cosine else Q
        assert got[4].tolist() == list(paths), "%s: paths %s, the model %s" % (what, got[4].tolist(), list(paths))
        for self.qi in range(Q.shape[0]):
            assert got[3][self.qi, 3] == 0, "%s: status %d" % (what, got[3][self.qi, 3])
            compare_row(got, self.qi, self.want(Qr[self.qi], n, ef, adms[self.qi], paths[self.qi]), n, what)
        self.qi = None

    # ---- checks ----
    def check(self, c):
        m = self.m
        if m.after:
            m.ev["check_after:%s" % m.after] += 1
            m.after = None
        self.n_checks += 1
        fam = c["family"]
        if fam in HOST_FAMILIES:
            return self.check_host_family(c)
        if fam in ANCHORS:
            m.note("state:%s:%s" % (fam, "del" if m.deleted.any() else "nodel"))
        if fam in COMPOSITE_FAMILIES:
            if self.product == "gpu":
                self.index.set_option("filter_exact_max", c["exact_max"])
            m.option("filter_exact_max", c["exact_max"])
            return self.check_composite(c)
        nq = c["Q"].shape[0]
        setname, keys, ranges, masks = c.get("set"), c.get("keys"), c.get("ranges"), c.get("masks")
        exact_max = c["exact_max"]
        gpu = self.product == "gpu"
        if gpu:
            self.index.set_option("filter_exact_max", exact_max)
        m.option("filter_exact_max", exact_max)
        Q, n, ef = c["Q"], c["n"], c["ef"]
        s = self.sets.get(setname)
        lo = hi = None
        if ranges is not None and fam != "ranges":
            lo = np.array([r[0][0] for r in ranges], dtype=np.uint32)
            hi = np.array([r[0][1] for r in ranges], dtype=np.uint32)

        def note(paths, family=fam):
            for p in set(paths):
                m.ev["path%d:%s" % (p, family)] += 1

        if fam in DEVICE_FAMILIES:
            # the device form first (its own syncs are what is held to the model), then the host form with
            # filter_exact_max = -1, which it must equal
            m.option("filter_exact_max", -1)
            d_dev = m.device_call(setname, ranges is not None)
            adms, paths, d_host = m.plan(nq, setname, keys, ranges, None)
            note(paths)
            if not gpu:
                return
            from tests.test_gpu_mask_set import same
            self.index.set_option("filter_exact_max", -1)
            before = self.stats()
            if fam == "set_device":
                from tests.test_gpu_mask_set import device_call
                code, dev = device_call(self.index, s, Q, n, ef, np.array(keys))
            elif fam == "range_device":
                from tests.test_gpu_labels import device_call
                code, dev = device_call(self.index, Q, n, ef, lo, hi)
            else:
                from tests.test_gpu_filtered_set_range import device_call
                code, dev = device_call(self.index, s, Q, n, ef, np.array(keys), lo, hi)
            self.expect_delta(before, d_dev, "device form")
            assert code is None, "the device form ended with status %s" % code
            self.compare(dev, Q, n, ef, adms, paths, "device form")
            before = self.stats()
            host = self.host_call(fam.replace("_device", ""), c, s, lo, hi)
            self.expect_delta(before, d_host, "host form after the device form")
            same(dev, host, "device form against host form")
            return
        if fam == "brute_force":
            if m.deleted.any():
                adms, paths, d = m.plan(nq, exact_only=True)
            else:
                adms, paths, d = [m.live()] * nq, [1] * nq, zero_delta()
                d["uploads"] = m.ensure_uploaded()
            if not gpu:
                return
            from tests import filtered_restate as FR
            before = self.stats()
            ids, dists = self.index.brute_force(Q, n)
            self.expect_delta(before, d, fam)
            Qr = unit(Q) if self.cosine else Q
            for self.qi in range(nq):
                w = FR.exact(self.ridx(), Qr[self.qi], n, np.flatnonzero(adms[self.qi]))
                assert np.array_equal(ids[self.qi], w["ids"]), (ids[self.qi], w["ids"])
                assert np.array_equal(dists[self.qi].view(np.uint32), w["dists"].view(np.uint32))
            return
        if fam == "search_batch" or (fam == "grouped" and not m.deleted.any()):
            filtered = bool(m.deleted.any())
        else:
            filtered = True
        one = fam in ("one", "one_threads")
        if one and ranges is None:
            ranges = [[FULL]] * nq
        if filtered:
            adms, paths, d = m.plan(nq, setname, keys if (setname or masks) else None, ranges, masks,
                                    one_query=one)
        else:
            adms, paths, d = [m.live()] * nq, [0] * nq, zero_delta()
            d["uploads"] = m.ensure_uploaded()
        if fam.startswith("grouped"):
            d["label_words_uploaded"] += m.sync_labels() if ranges is None else 0  # (the collapse reads the labels)
        note(paths)
        if not gpu:
            return
        import hnsw_rs_amd as H
        before = self.stats()
        if fam == "search_batch":
            pk = ("deleted_queries_graph", "deleted_queries_exact", "deleted_overflow_exact")
            p0 = [self.index.stat(k) for k in pk]
            with H.kernel_log() as log:
                ids, dists, counts, stats = self.index.search_batch(Q, n, ef)
            self.expect_delta(before, d, fam)
            moved = [self.index.stat(k) - v for k, v in zip(pk, p0)]
            if filtered:
                assert moved == [paths.count(0), paths.count(1), 0], "queries by path %s, the model's paths %s" % (moved, paths)
                self.compare((ids, dists, counts, stats, np.array(paths, dtype=np.uint8)), Q, n, ef, adms, paths, fam)
            else:
                from oracle import restate_np as R
                from tests.util import assert_search_equal
                assert moved == [0, 0, 0]
                bad = [k for k in log if k.startswith("hx_filt") or k.startswith("hx_deleted")]
                assert not bad, "nothing is deleted, and the kernel log shows %s" % bad
                Qr = unit(Q) if self.cosine else Q
                assert_search_equal((ids, dists, counts, stats), self.orc().search_batch(Qr, n, ef), "against the oracle")
                for self.qi in range(nq):
                    w_ids, w_d, w_c = R.ann_by_vector(self.ridx(), Qr[self.qi], n, ef)
                    assert counts[self.qi] == len(w_ids) and np.array_equal(ids[self.qi, : len(w_ids)], w_ids)
                    assert np.array_equal(dists[self.qi, : len(w_ids)].view(np.uint32), w_d.view(np.uint32))
                    assert tuple(int(x) for x in stats[self.qi, :3]) == tuple(w_c)
            return
        if fam.startswith("grouped"):
            return self.check_grouped(c, s, lo, hi, adms, paths, d, before, filtered)
        if fam == "one":
            o_ids, o_d, o_c, o_p = self.index.search_filtered(Q[0], n, ef, lo[0] if lo is not None else 0,
                                                              hi[0] if hi is not None else MAX, s,
                                                              keys[0] if s is not None else None)
            self.expect_delta(before, d, fam)
            self.compare_one([(o_ids, o_d, o_c, o_p)], Q, n, ef, adms, paths)
            return
        if fam == "one_threads":
            out, errs = [None] * nq, []
            gate = threading.Barrier(nq)

            def call(i):
                try:
                    gate.wait()
                    out[i] = self.index.search_filtered(Q[i], n, ef, lo[i] if lo is not None else 0,
                                                        hi[i] if hi is not None else MAX, s,
                                                        keys[i] if s is not None else None)
                except Exception as e:  # (reported below, from the test's thread)
                    errs.append((i, e))
            ts = [threading.Thread(target=call, args=(i,)) for i in range(nq)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, "a thread's call failed: %s" % errs
            self.expect_delta(before, d, fam)
            self.compare_one(out, Q, n, ef, adms, paths)
            return
        got = self.host_call(fam, c, s, lo, hi)
        self.expect_delta(before, d, fam)
        self.compare(got, Q, n, ef, adms, paths, fam)

    def host_call(self, fam, c, s, lo, hi):
        index, Q, n, ef = self.index, c["Q"], c["n"], c["ef"]
        if fam == "filtered":
            return index.search_batch_filtered(Q, n, ef, c["masks"][0])
        if fam == "multi":
            return index.search_batch_filtered_multi(Q, n, ef, c["masks"], np.array(c["keys"]))
        if fam == "set":
            return index.search_batch_filtered_set(Q, n, ef, s, np.array(c["keys"]))
        if fam == "range":
            return index.search_batch_filtered_range(Q, n, ef, lo, hi)
        if fam == "ranges":
            return index.search_batch_filtered_ranges(Q, n, ef, c["ranges"])
        if fam == "set_range":
            return index.search_batch_filtered_set_range(Q, n, ef, s, np.array(c["keys"]), lo, hi)
        raise ValueError(fam)

    def compare_one(self, outs, Q, n, ef, adms, paths):
        """hnsw_search_filtered's answers (ids, dists, count, path; it returns no counters)"""
        from tests import filtered_restate as FR
        Qr = unit(Q) if self.cosine else Q
        for self.qi, (ids, dists, count, path) in enumerate(outs):
            assert path == paths[self.qi], "path %d, the model %d" % (path, paths[self.qi])
            w_ids, w_d, w_c = FR.padded(self.want(Qr[self.qi], n, ef, adms[self.qi], paths[self.qi]), n)
            assert count == w_c, (count, w_c)
            assert np.array_equal(ids, w_ids), (ids, w_ids)
            assert np.array_equal(dists.view(np.uint32), w_d.view(np.uint32))
        self.qi = None

    def check_grouped(self, c, s, lo, hi, adms, paths, d, before, filtered):
        from hnsw_rs_amd.grouped import group_by_label
        from oracle import restate_np as R
        from tests import filtered_restate as FR
        from tests import grouped_cases as GC
        Q, ef, pool, G, P = c["Q"], c["ef"], c["pool"], c["G"], c["P"]
        nq = Q.shape[0]
        got = self.index.search_batch_grouped(Q, G, P, pool, ef, s, np.array(c["keys"]) if s is not None else None, lo, hi)
        self.expect_delta(before, d, c["family"])
        Qr = unit(Q) if self.cosine else Q
        c_ids = np.full((nq, pool), MAX, dtype=np.uint32)
        c_d = np.full((nq, pool), np.inf, dtype=np.float32)
        c_n = np.zeros(nq, dtype=np.uint32)
        for self.qi in range(nq):
            if filtered:
                w = self.want(Qr[self.qi], pool, ef, adms[self.qi], paths[self.qi])
            else:
                w_ids, w_d, w_c = R.ann_by_vector(self.ridx(), Qr[self.qi], pool, ef)
                w = dict(ids=w_ids, dists=w_d, counters=w_c)
            c_ids[self.qi], c_d[self.qi], c_n[self.qi] = FR.padded(w, pool)
            assert got[5][self.qi, 3] == 0, "status %d" % got[5][self.qi, 3]
            assert tuple(int(x) for x in got[5][self.qi, :3]) == tuple(w["counters"]), (got[5][self.qi], w["counters"])
        self.qi = None
        want = group_by_label(c_ids, c_d, c_n, self.m.labels, G, P)
        GC.assert_grouped_equal(got, want, c["family"])

    # ---- the search-then-post-process entry points (lists_host.h) ----
    def feature_stats(self):
        return {k: self.index.stat(k) for k in FEATURE_COUNTERS}

    def expect_features(self, before, want, what):
        got = {k: self.index.stat(k) - v for k, v in before.items()}
        full = {k: want.get(k, 0) for k in FEATURE_COUNTERS}
        assert got == full, "%s: the feature counters moved by %s, expected %s" % (what, got, full)

    def stored_row(self, i):
        """the row of an id as hnsw_get_vector returns it, by the oracle (under the cosine option: the stored unit row)"""
        v = self.orc().get_vals(i).copy()
        if i in self.tamper_rows:
            e, ulps = self.tamper_rows[i]
            for _ in range(ulps):
                v[e] = np.nextafter(v[e], np.float32(np.inf))
        return v

    def late_labels(self):
        lab = self.m.labels.copy()
        for i, v in self.tamper_labels.items():
            if i < lab.size:
                lab[i] = v
        return lab

    def cand_lists(self, V, n, ef, adms, paths, host_form):
        """the candidate lists of the rows of V (as the search stages them: unit length under the cosine option) with
        n and ef as the entry point hands them on: under the model's predicate and planned path in the host form, the
        reference's own walk otherwise -> ids [rows, n], dists, counts, stats int64 [rows, 4]"""
        from oracle import restate_np as R
        from tests import filtered_restate as FR
        rows = V.shape[0]
        ids = np.full((rows, n), MAX, dtype=np.uint32)
        dists = np.full((rows, n), np.inf, dtype=np.float32)
        counts = np.zeros(rows, dtype=np.uint32)
        stats = np.zeros((rows, 4), dtype=np.int64)
        seen = {}
        for r in range(rows):
            key = (V[r].tobytes(), paths[r], adms[r].tobytes() if host_form else b"")
            if key not in seen:
                if host_form:
                    w = self.want(V[r], n, ef, adms[r], paths[r])
                else:
                    w_ids, w_d, w_c = R.ann_by_vector(self.ridx(), V[r], n, ef)
                    w = dict(ids=w_ids, dists=w_d, counters=w_c)
                seen[key] = w
            w = seen[key]
            ids[r], dists[r], counts[r] = FR.padded(w, n)
            stats[r, :3] = w["counters"]
        return ids, dists, counts, stats

    def composite_call(self, c):
        """the product's call of a composite check"""
        index, fam, pool, ef = self.index, c["family"], c["pool"], c["ef"]
        if fam == "radius":
            return index.search_batch_radius(c["Q"], c["radius"], c["n_first"], pool, ef)
        if fam.startswith("diverse"):
            s, ranges = self.sets.get(c.get("set")), c.get("ranges")
            lo = None if ranges is None else np.array([r[0][0] for r in ranges], dtype=np.uint32)
            hi = None if ranges is None else np.array([r[0][1] for r in ranges], dtype=np.uint32)
            return index.search_batch_diverse(c["Q"], c["n"], pool, ef, c["lam"], s,
                                              np.array(c["keys"]) if s is not None else None, lo, hi)
        if fam == "from_rows":
            return index.search_batch_from_rows(c["src"], c.get("weights"), c["n"], ef, c["exclude"])
        if fam == "by_id":
            return index.search_batch_by_id(c["src"][:, 0], c["n"], ef, c["exclude"])
        if fam == "multi_vec":
            return index.search_batch_multi(c["Q"], c["n"], pool, ef, c.get("weights"), ("sum", "min")[c["mode"]])
        if fam == "late":
            return index.search_batch_late(c["Q"], c["n"], pool, ef, ("sum", "sum_sq")[c["mode"]])
        raise ValueError(fam)

    def refused_call(self, c):
        """the call at the host form's limit + 1: HnswError with ERR_ARG, and no counter moves"""
        import hnsw_rs_amd as H
        from hnsw_rs_amd import _lib
        before, f_before = self.stats(), self.feature_stats()
        raised = None
        try:
            self.composite_call(c)
        except H.HnswError as e:
            raised = e
        assert raised is not None, "the call beyond the host form's limit was answered"
        assert raised.code == _lib.ERR_ARG, "the refused call raised %s" % raised
        self.expect_delta(before, zero_delta(), "refused call")
        self.expect_features(f_before, {}, "refused call")
        self.m.note("held_refused:%s" % c["family"])

    def check_composite(self, c):
        m, fam, gpu = self.m, c["family"], self.product == "gpu"
        deleted = bool(m.deleted.any())
        host_form = deleted or fam in FILTERED_COMPOSITES
        if c.get("refused"):
            assert host_form, "a refused call was drawn for the device form"
            m.note("refused:%s" % fam)
            if gpu:
                self.refused_call(c)
            return
        m.note("state:%s:%s" % (fam, "del" if deleted else "nodel"))
        if not deleted and m.seen_zero:
            m.note("none_deleted_after_some:%s" % fam)
        d_total = zero_delta()

        def plan(n_rows):
            """the candidate call of n_rows queries through the model -> admissible, paths; its deltas are added up"""
            if host_form:
                adms, paths, d = m.plan(n_rows, c.get("set"), c.get("keys") if c.get("set") else None, c.get("ranges"))
                for p in set(paths):
                    m.note("hpath%d:%s" % (p, fam))
            else:
                adms, paths, d = [m.live()] * n_rows, [0] * n_rows, zero_delta()
                d["uploads"] = m.ensure_uploaded()
            for k in COUNTERS:
                d_total[k] += d[k]
            return adms, paths

        def note_patched(ids, seen=""):
            if any(int(i) in m.patched for i in ids):
                m.note("%spatched:%s" % (seen, fam))
                if m.inline_rows == 1:
                    m.note("%spatched_inline:%s" % (seen, fam))

        if fam == "radius":
            return self.check_radius(c, host_form, plan, note_patched, d_total)
        pool, ef = c["pool"], c["ef"]
        rows_m = unit(m.vecs) if self.cosine and m.len else m.vecs
        src = weights = None
        if fam in ("from_rows", "by_id"):
            src, weights = c["src"], c.get("weights")
            nq, width = src.shape
            n_cand, ef_c = (c["n"] + width if c["exclude"] else c["n"]), ef
            if self.product is not None:
                from hnsw_rs_amd.from_rows import compose_rows
                V, st = compose_rows(src, weights, self.stored_row, m.len)
                assert (st == 0).all(), "a drawn query has no legal source"
            else:  # (for the model's events alone: the rows composed out of the model's vectors)
                V = np.zeros((nq, m.d), dtype=np.float32)
                for q in range(nq):
                    for s in range(width):
                        if src[q, s] != MAX:
                            V[q] += (np.float32(1) if weights is None else weights[q, s]) * rows_m[src[q, s]]
        elif fam in ("multi_vec", "late"):
            nq, T = c["Q"].shape[:2]
            V = c["Q"].reshape(nq * T, -1)
            n_cand, ef_c = pool, max(ef, pool, 1)
        else:
            nq, V = c["Q"].shape[0], c["Q"]
            n_cand, ef_c = pool, ef
        adms, paths = plan(V.shape[0])
        sure = [m.nearest(V[r], min(SURE, n_cand), adms[r], self.cosine) for r in range(V.shape[0])]
        patched = set(m.patched)

        def note_lists(lists, seen=""):
            """what the lists of a check go through: `lists` one set of candidate ids per row"""
            if any(i in patched for s in lists for i in s) or (src is not None and set(src[src != MAX].tolist()) & patched):
                m.note("%spatched:%s" % (seen, fam))
                if m.inline_rows == 1:
                    m.note("%spatched_inline:%s" % (seen, fam))
            if fam not in ("multi_vec", "late"):
                return
            for q in range(nq):
                per = lists[q * T:(q + 1) * T]
                pairs = [(per[a], per[b]) for a in range(T) for b in range(a + 1, T)]
                if fam == "multi_vec" and any(a & b for a, b in pairs):
                    m.note("%smulti_vec:one_id_in_two_lists" % seen)
                if fam == "late" and any(i != j and m.labels[i] == m.labels[j] for a, b in pairs for i in a for j in b):
                    m.note("%slate:shared_document" % seen)
            if fam == "late":
                every = {i for s in lists for i in s}
                if any(i >= column for i in every):
                    m.note("%slate:beyond_the_column" % seen)
                if label_copy_moved and every & changed:
                    m.note("%slate:label_changed" % seen)

        if fam == "late":
            # the label column as the call finds it: the ids its words cover, the ids whose label changed since it last
            # went to HBM, and whether this call's sync sends changed words (lab:scatter, lab:whole)
            column, changed = 2 * m.lab_nw, set(m.lab_changed)
            moved = (m.ev["lab:scatter"], m.ev["lab:whole"])
            d_total["label_words_uploaded"] += m.sync_labels()  # (the scoring reads the labels)
            label_copy_moved = moved != (m.ev["lab:scatter"], m.ev["lab:whole"])
        note_lists([{int(i) for i in s} for s in sure])
        if self.product is None:
            return
        # with the library at hand the candidate lists are known without a GPU (the graph is the host's): what they go
        # through is noted a second time, as seen
        Vr = unit(V) if self.cosine else V
        ids, dists, counts, stats = self.cand_lists(Vr, n_cand, ef_c, adms, paths, host_form)
        note_lists([{int(i) for i in ids[r, :counts[r]]} for r in range(ids.shape[0])], "seen:")
        if not gpu:
            return
        from hnsw_rs_amd import diverse, from_rows, late, multi
        from tests import diverse_cases as DC
        from tests import from_rows_cases as FC
        from tests import late_cases as LC
        from tests import multi_cases as MC
        orc = self.orc()
        if fam.startswith("diverse"):
            want = diverse.mmr_select(ids, dists, counts, None, orc.distance, c["lam"], c["n"])
            features = {"diverse_calls": 1, "diverse_launches": 1}
        elif src is not None:
            want = from_rows.drop_ids(ids, dists, counts, None, src, c["n"]) if c["exclude"] else (ids, dists, counts)
            features = {"from_rows_calls": 1, "from_rows_compose_launches": 1, "from_rows_drop_launches": int(c["exclude"])}
        elif fam == "multi_vec":
            want = multi.fuse_lists(Vr.reshape(nq, T, -1), c.get("weights"), ("sum", "min")[c["mode"]],
                                    ids.reshape(nq, T, pool), counts.reshape(nq, T), None, orc.distance_batch, c["n"], m.len)
            features = {"multi_calls": 1, "multi_fuse_launches": 1}
        else:
            want = late.late_interaction(Vr.reshape(nq, T, -1), ("sum", "sum_sq")[c["mode"]], ids.reshape(nq, T, pool),
                                         counts.reshape(nq, T), None, orc.distance_batch, self.late_labels(), c["n"], m.len)
            features = {"late_calls": 1, "late_launches": 1}
        before, f_before = self.stats(), self.feature_stats()
        got = self.composite_call(c)
        self.expect_delta(before, d_total, fam)
        self.expect_features(f_before, features, fam)
        g_stats = got[-1]
        if fam.startswith("diverse"):
            DC.assert_diverse_equal(got, want, fam)
        elif src is not None:
            FC.assert_drop_equal(got[:3], want[:3], fam)
        elif fam == "multi_vec":
            MC.assert_fused_equal(got[:4] + (g_stats[:, 3],), want, fam)
        else:
            LC.assert_late_equal(got[:6] + (g_stats[:, 3],), want, fam)
        if fam in ("multi_vec", "late"):  # (the counters of a query's T searches, summed)
            stats = stats.reshape(nq, T, 4).sum(axis=1)
        assert np.array_equal(g_stats[:, :3], stats[:, :3]), "%s: counters %s, the candidates' %s" % (fam, g_stats[:, :3], stats[:, :3])
        assert (g_stats[:, 3] == 0).all(), "%s: statuses %s" % (fam, g_stats[:, 3])
        m.note("held:%s" % fam)

    def check_radius(self, c, host_form, plan, note_patched, d_total):
        m, gpu = self.m, self.product == "gpu"
        Q, n_first, max_n, ef = c["Q"], c["n_first"], c["pool"], c["ef"]
        nq = Q.shape[0]
        radius = np.broadcast_to(np.asarray(c["radius"], dtype=np.float32), (nq,))
        n_of = [n_first]  # the n of every rung of the ladder
        while n_of[-1] < max_n:
            n_of.append(min(2 * n_of[-1], max_n))
        K = len(n_of)
        # what the model alone says of the ladder: the rows within a radius counted in float64, with a margin on both
        # sides for what f32 and the 8-bit codes round; a query whose two counts leave at the same rung is predicted
        live = m.live()
        n_live = int(live.sum())
        exits = []
        for q in range(nq):
            d, r = m.dist64(Q[q], self.cosine)[live], float(radius[q])
            with np.errstate(invalid="ignore"):
                w = [min(n_live, int((d <= x).sum())) for x in (max(r * 0.95 - 0.02, 0.0), r * 1.05 + 0.02)]
            a, b = [next(k for k in range(K) if x < n_of[k] or k == K - 1) for x in w]
            exits.append(b)
            if a == b and K >= 3:
                m.note("radius:leaves_%s" % ("first" if a == 0 else "last" if a == K - 1 else "middle"))
            if a == b == K - 1 and w[0] >= max_n:
                m.note("radius:truncated")
        if self.product is None:
            for k in range(max(exits) + 1):  # (every rung is a search of its own under the planner)
                adms, _ = plan(nq)
                if k == 0:
                    note_patched([i for q in range(nq) for i in m.nearest(Q[q], min(SURE, n_first), adms[q], self.cosine)])
            return
        # with the library at hand the ladder is known without a GPU (the graph is the host's): what it goes through is
        # noted a second time, as seen
        from hnsw_rs_amd.radius import radius_ladder
        from tests import radius_cases as RC
        rung = [0]

        def search(Qs, n, ef_k):
            adms, paths = plan(Qs.shape[0])
            lists = self.cand_lists(Qs, n, ef_k, adms, paths, host_form)
            if rung[0] == 0:
                note_patched([i for q in range(nq) for i in m.nearest(Q[q], min(SURE, n_first), adms[q], self.cosine)])
                note_patched([i for q in range(nq) for i in lists[0][q, :lists[2][q]]], "seen:")
            rung[0] += 1
            return lists

        want = radius_ladder(search, unit(Q) if self.cosine else Q, radius, n_first, max_n, ef)
        for q in range(nq):
            k = int(want[4][q]) - 1
            if K >= 3:
                m.note("seen:radius:leaves_%s" % ("first" if k == 0 else "last" if k == K - 1 else "middle"))
            if want[3][q] & 1:
                m.note("seen:radius:truncated")
        if not gpu:
            return
        before, f_before = self.stats(), self.feature_stats()
        got = self.composite_call(c)
        self.expect_delta(before, d_total, "radius")
        self.expect_features(f_before, {"radius_calls": 1, "radius_rungs": rung[0], "radius_launches": rung[0]}, "radius")
        RC.assert_ladder_equal(got, want, "radius")
        m.note("held:radius")

    def check_host_family(self, c):
        m, fam = self.m, c["family"]
        if fam == "count_labels":
            want = m.count_labels(c["members"])
            if self.product is not None:
                got = self.index.count_labels_in_ranges(c["members"])
                assert got == want, "count_labels_in_ranges(%s) = %d, the model %d" % (c["members"], got, want)
        # (deleted_ids, get_labels, MaskSet.read and MaskSet.count are held to the model after every op: check_host_state)


def replay(seed, kind, upto, product="gpu", steps=None, cosine=False, families="default"):
    """re-runs the first `upto` ops of a schedule (a failure names its step index: the prefix is found by hand)"""
    return Machine(seed, kind, product, steps, cosine, families).run(upto)
