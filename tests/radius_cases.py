"""Shared builders of the radius search tests (tests/test_radius_host.py, tests/test_gpu_radius.py): a deliberately naive
cut, adversarial candidate lists, the ladder worlds with their radii, and the coverage condition.  Importable without a
GPU: nothing here touches the product library's device side."""
import functools

import numpy as np

from oracle import oracle_py as O
from tests.util import rand_vectors

MAX = 0xFFFFFFFF
MORE = 1
NQ = 14  # queries of the adversarial lists
N_INS = (1, 63, 64, 65, 200, 1024)
RANKS = (0, 3, 7, 8, 20, 60, 127, 168)
N_FIRST, MAX_N, EF = 8, 128, 16  # the ladder's arguments


# ---- the cut, one entry at a time ------------------------------------------------------------------------------------
def naive_cut(ids, dists, counts, stats, radius, n_out):
    """THE CUT of include/hnsw_mi355x.h as a plain loop -> ids, dists, counts, flags"""
    nq, n_in = ids.shape
    o_ids = np.full((nq, n_out), MAX, dtype=np.uint32)
    o_dists = np.full((nq, n_out), np.inf, dtype=np.float32)
    o_counts, o_flags = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        if stats is not None and stats[q, 3] != 0:
            continue
        r = np.float32(radius[q])
        n_present = w = 0
        for j in range(n_in):
            present = j < min(int(counts[q]), n_in) if counts is not None else ids[q, j] != MAX
            if not present:
                continue
            n_present += 1
            d = dists[q, j]
            if not (np.isnan(d) or np.isnan(r)) and d <= r:
                o_ids[q, w] = ids[q, j]
                o_dists[q, w] = d
                w += 1
        o_counts[q] = w
        o_flags[q] = MORE if n_present == n_in and w == n_present else 0
    return o_ids, o_dists, o_counts, o_flags


def adversarial_lists(n_in, with_counts, seed):
    """NQ unsorted candidate lists of n_in entries with their radii and stats -> ids, dists, counts or None, stats int64
    [NQ, 4], radius.  Planted: q0 all present, radius +inf (the flag); q1 radius 0 with some distances 0; q2 radius an
    exact tie with an entry; q3 a failed status; q4 NaN distances inside a +inf radius (no flag); q5 nothing present;
    q6 radius below every distance; q7 a NaN radius; the rest random counts or absent entries in the middle."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 2 ** 32 - 1, (NQ, n_in), dtype=np.uint64).astype(np.uint32)
    ids[ids == MAX] = 0
    dists = rng.random((NQ, n_in), dtype=np.float32) * np.float32(4.0)
    dists[rng.random((NQ, n_in)) < 0.1] = np.float32(0.0)
    radius = np.quantile(dists, 0.5, axis=1).astype(np.float32)
    counts = None
    if with_counts:
        counts = rng.integers(0, n_in + 2, NQ).astype(np.uint32)  # (n_in + 1: a count beyond the list)
        counts[[0, 1, 2, 4]] = n_in
        counts[5] = 0
    else:
        gone = rng.random((NQ, n_in)) < 0.3
        gone[[0, 1, 2, 4]] = False
        gone[5] = True
        ids[gone] = MAX
    radius[0] = np.inf
    radius[1] = 0.0
    radius[2] = dists[2, n_in // 2]
    dists[2, 0] = dists[2, n_in // 2]  # (two entries at the radius when n_in > 1)
    dists[4, ::3] = np.nan
    radius[4] = np.inf
    radius[6] = np.float32(-1.0)
    radius[7] = np.nan
    radius[8] = np.inf  # with random presence: full only by chance
    stats = rng.integers(2 ** 31, 2 ** 32, (NQ, 4)).astype(np.int64)
    stats[:, 3] = 0
    stats[3, 3] = -2  # HNSW_ERR_NAN_INPUT
    for a in (ids, dists, stats, radius) + (() if counts is None else (counts,)):
        a.setflags(write=False)
    return ids, dists, counts, stats, radius


def assert_cut_equal(got, want, what):
    """ids, distance BITS, counts and flags"""
    assert np.array_equal(got[2], want[2]), what + ": counts differ"
    assert np.array_equal(got[3], want[3]), what + ": flags differ"
    assert np.array_equal(got[0], want[0]), what + ": ids differ"
    assert np.array_equal(np.asarray(got[1]).view(np.uint32), np.asarray(want[1]).view(np.uint32)), what + ": distance bits differ"


def assert_ladder_equal(got, want, what):
    """ids, distance bits, counts, flags, rungs and the counters and status of the stats"""
    assert_cut_equal(got, want, what)
    assert np.array_equal(got[4], want[4]), what + ": rungs differ"
    g, w = np.asarray(got[5]).astype(np.int64), np.asarray(want[5]).astype(np.int64)
    assert np.array_equal(g[:, :3] & 0xFFFFFFFF, w[:, :3] & 0xFFFFFFFF) and np.array_equal(g[:, 3], w[:, 3]), what + ": stats differ"


# ---- the ladder worlds ----------------------------------------------------------------------------------------------
WORLDS = {"small": (3000, 16, 8, False), "lean": (2000, 100, 16, False), "ties": (3000, 16, 8, True)}


@functools.lru_cache(maxsize=None)
def world(name, kind):
    """-> rows, levels, the oracle index, 64 queries (the first 8 equal to stored rows) and their radii: query i the
    exact distance, in the kind's own arithmetic, of its true neighbour of rank RANKS[i % 8], every 16th query half its
    nearest distance instead.  "ties": the last 200 rows duplicate the first 200."""
    N, d, m, dup = WORLDS[name]
    rows = np.random.default_rng(1).standard_normal((N, d)).astype(np.float32)
    if dup:
        rows[-200:] = rows[:200]
    levels = O.draw_levels(N, m, 7)
    orc = O.OracleHNSW(m, 32, d, kind).insert_bulk(rows, levels)
    Q = np.random.default_rng(2).standard_normal((64, d)).astype(np.float32)
    Q[:8] = rows[:8]
    _, true_d = orc.brute_force(Q, RANKS[-1] + 1, nthreads=8)
    radius = np.array([true_d[i, RANKS[i % 8]] for i in range(64)], dtype=np.float32)
    radius[15::16] = true_d[15::16, 0] * np.float32(0.5)  # (queries 15, 31, 47, 63: none of them a stored row)
    for a in (rows, levels, Q, radius):
        a.setflags(write=False)
    return rows, levels, orc, Q, radius


def classes(want):
    """the coverage classes of a ladder answer -> dict of query counts"""
    ids, dists, counts, flags, rungs, stats = want
    trunc = (flags & MORE) != 0
    return {"empty": int((counts == 0).sum()),
            "rung0": int(((rungs == 1) & (counts > 0) & ~trunc).sum()),
            "deep": int(((rungs >= 3) & ~trunc).sum()),
            "truncated": int(trunc.sum())}


def assert_covered(want, what):
    """the coverage condition: at least 4 queries empty, finished non-empty at rung 0, finished at rung >= 2
    untruncated, and truncated -- on the EXPECTED values, so that a test cannot pass vacuously"""
    c = classes(want)
    assert all(v >= 4 for v in c.values()), (what, c)


# ---- the hub graph (tests/test_gpu_parity.py, test_device_pointer_entry_recovers_from_a_full_visited_table) ----------
@functools.lru_cache(maxsize=None)
def hub_world(kind):
    """that test's graph, built the same way: node 5 gets 5000 more neighbours on layer 0, which fills the default
    visited table of a query that expands it -> rows, levels, the oracle index holding the graph"""
    n, d, m = 9000, 100 if kind == O.VEC_F32 else 12, 4
    vs, lv = rand_vectors(n, d, 13), O.draw_levels(n, m, 3)
    orc = O.OracleHNSW(m, None, d, kind).insert_bulk(vs, lv)
    ids, offs, nbrs = orc.layer_csr(0)
    adj = {int(i): set(int(x) for x in nbrs[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)}
    for t in range(100, 5100):
        adj[5].add(t)
        adj[t].add(5)
    rows = [sorted(adj[int(i)]) for i in ids]
    orc2 = O.OracleHNSW(m, None, d, kind)
    orc2.import_points(vs, lv)
    orc2.import_layer(0, ids, np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64),
                      np.concatenate([np.array(r, dtype=np.uint32) for r in rows]))
    for l in range(1, orc.nb_layers):
        orc2.import_layer(l, *orc.layer_csr(l))
    orc2.set_ep(orc.ep)
    return vs, lv, orc2
