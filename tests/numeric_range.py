"""Every distance routine at the edges of f32's range: the recipes that put a fixture's data there, the table of calls
(one per distance routine, selected from tests/kernel_matrix.py by a rule) and the runner that holds each call to the
CPU oracle.  tests/test_gpu_numeric_range.py runs the table on an MI355X (an environment group in a child process of
its own, `python -m tests.numeric_range <group>`); tests/test_numeric_range_host.py checks, without a GPU, that the
recipes do what they claim and that the oracle itself is right there.

Fixtures.  KM.fixture(kind, d, m) gives the rows `vs` and a host-built graph at scale 1.  A recipe multiplies the rows
by a scale derived (float64) from the fixture's own query-to-row distances and imports them, with the same levels and
the scale-1 graph, into a product index and an oracle (any graph serves a parity test; building one from subnormal
rows would take the CPU half a minute).  The oracle quantises the scaled rows itself.

  sub    2^k, k the largest integer that puts the largest query-to-row distance below 2^-64: every squared sum is
         subnormal and non-zero, every distance is in (0, 2^-63).  A routine that flushed subnormals would return 0
         everywhere and order by id.
  under  2^(k - 5): the squared sums have a handful of bits left, so every ef-100 list holds bit-equal distances
         (ties decided by id) while the rows still have many distinct distances.
  over   sqrt(FLT_MAX / q), q the p-quantile of the squared distances (p = OVER_P, 0.03 unless a fixture needs another):
         for most queries the sum overflows for some rows and not for others, and a list mixes finite and +inf keys.

Queries.  KM.queries(c, vs) times the scale, then five more, unscaled unless stated: (a) every component -0.0, (b)
components alternating +0.0 / -0.0, (c) vs[5] times the scale times 2^-50 (subnormal inputs; 8-bit: a subnormal delta
in the query quantiser), (d) components alternating +3e38 / -3e38 (f32: every distance +inf; 8-bit: hi - lo overflows),
(e) the scaled vs[7] with component 0 replaced by +inf.  What each of the queries behind the base ones must give is
taken from the oracle, run on that query alone: where the oracle raises, the product must report an error status and
count 0 for that query alone inside the batch (entry points without a per-query status: an error for that query alone),
where it answers, the product must give its answer.

Runner.  The queries the oracle answers go through KM.run_call unchanged (the same kernel-log condition, ids, distance
bits, counts and counters).  Then the whole batch, the raising queries included, goes through the entry point once
more: the status column 0 for every query the oracle answered, an error status and count 0 exactly where it raised,
every other row as before.

brute_fast (hx_brute_mfma_kernel + hx_pair_distance_kernel) has no row here: its contract is its own, see
run_brute_fast.
"""
import contextlib
import math
import os
import re
import sys

import numpy as np

from tests import kernel_matrix as KM
from tests.kernel_matrix import F32, N_POINTS, N_QUERIES, Call

RECIPES = ("sub", "under", "over")
FLT_MAX = float(np.finfo(np.float32).max)
# `over`: the quantile of the squared distances that goes to FLT_MAX, per fixture (kind, d, m) where 0.03 misses the
# condition of tests/test_numeric_range_host.py (at least half of the base queries' ef-100 lists mix finite and +inf)
OVER_P = {}

# ---- the table -------------------------------------------------------------------------------------------------------
# A distance routine is a kernel family with its template arguments minus the list width (the position below): the
# distance code of hx_search_kernel<KIND, P, DS, R, FAT> is the same for every R.  A family not listed has no width.
WIDTH_ARG = {"hx_search_kernel": 3, "hx_lean_q8_kernel": 0, "hx_lean_f32_kernel": 1, "hx_pair_f32_kernel": 1,
             "hx_filt_graph_kernel": 3}
# entry points the runner knows (the selection takes no "device" call: its rows have a "batch" call at the same ef)
ENTRIES = ("batch", "layer", "distance", "brute", "filtered", "filtered_exact", "brute_fast")


def routine_of(kernel):
    """'hx_search_kernel<1, 0, 0, 2, false>' -> ('hx_search_kernel', '1', '0', '0', 'false')"""
    m = re.match(r"(\w+)(?:<(.*)>)?$", kernel.strip())
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    if m.group(1) in WIDTH_ARG:
        del args[WIDTH_ARG[m.group(1)]]
    return (m.group(1),) + tuple(args)


def selection():
    """{routine(s) of a row: (the row's kernels, one call)}: per distinct routine the call whose ef is 100, else the
    one of the smallest ef; the first in table order among equals"""
    best = {}
    for row in KM.CASES:
        key = tuple(routine_of(k) for k in row.kernels)
        for c in row.calls:
            rank = (c.ef != 100, c.ef)
            if key not in best or rank < best[key][0]:
                best[key] = (rank, row.kernels, c)
    return {k: (kern, c) for k, (_, kern, c) in best.items()}


# dist_any_dim's f32 bulk stage (pairs > 0) needs d >= 128 in the generic form; the matrix's generic f32 fixture is d = 60
EXTRA = [((KM.S(F32, 0, 0, 2),), Call(F32, 200, 16, 0, "batch", 100, 100, N_QUERIES, "default", 0, (), ()))]
TABLE = [kc for kc in selection().values() if kc[1].entry != "brute_fast"] + EXTRA
BRUTE_FAST = [kc for kc in selection().values() if kc[1].entry == "brute_fast"]


def table_id(kc):
    return KM.call_id(kc[1])


# ---- recipes -----------------------------------------------------------------------------------------------------------

def base_queries(d, nq=N_QUERIES):
    """the base queries of KM.queries (its first c.nq rows), unscaled"""
    import hnsw_rs_amd as H
    return H.synth_rows(0, 0x3A7F9999 + d, 0, nq, d)


def squared_distances(Q, X):
    Q, X = Q.astype(np.float64), X.astype(np.float64)
    return np.maximum((Q * Q).sum(axis=1)[:, None] + (X * X).sum(axis=1)[None, :] - 2.0 * (Q @ X.T), 0.0)


def scale_of(recipe, kind, d, m, vs):
    """the recipe's factor as a float32 (module docstring); float64 from the fixture's own data"""
    Qb = base_queries(d)
    if recipe == "over":
        q = np.quantile(squared_distances(Qb, vs), OVER_P.get((kind, d, m), 0.03))
        return np.float32(math.sqrt(FLT_MAX / q))
    # the largest distance of the queries that are scaled: the base ones, the stored rows and the constant row
    Qs = np.concatenate([Qb, KM.edge_queries(vs, kind)[:3]])
    e = math.frexp(math.sqrt(squared_distances(Qs, vs).max()))[1]  # the distance is in [2^(e-1), 2^e)
    k = -64 - e
    return np.float32(2.0 ** (k if recipe == "sub" else k - 5))


def extra_queries(vs, s):
    """(a) .. (e) of the module docstring"""
    d = vs.shape[1]
    even = np.arange(d) % 2 == 0
    with np.errstate(over="ignore", under="ignore"):
        c = (vs[5] * s) * np.float32(2.0 ** -50)
        e = (vs[7] * s).astype(np.float32)
    e[0] = np.inf
    return np.stack([np.full(d, -0.0, np.float32), np.where(even, np.float32(0.0), np.float32(-0.0)), c,
                     np.where(even, np.float32(3e38), np.float32(-3e38)), e]).astype(np.float32)


_FIXTURES = {}


def fixture(kind, d, m, recipe):
    """(product index, oracle, scaled rows, scale): the scale-1 graph of KM.fixture over the recipe's rows"""
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    from tests.util import oracle_from_product
    key = (kind, d, m, recipe)
    if key not in _FIXTURES:
        idx1, _, vs = KM.fixture(kind, d, m)
        s = scale_of(recipe, kind, d, m, vs)
        rows = (vs * s).astype(np.float32)
        assert np.isfinite(rows).all() and (rows != 0).sum() == (vs != 0).sum(), (key, s)
        lv = O.draw_levels(N_POINTS, m, 0x3A7F + d)  # (KM.fixture's)
        idx = H.HNSW.new(m, 32, d, kind)
        idx.import_points(rows, lv)
        for l in range(idx1.nb_layers()):
            idx.import_layer(l, *idx1.get_layer(l).csr())
        idx.set_ep(int(idx1.params.ep))
        _FIXTURES[key] = (idx, oracle_from_product(idx, rows, lv), rows, s)
    return _FIXTURES[key]


def queries(c, vs, s):
    """KM.queries(c, vs) times the scale + (a) .. (e); the first c.nq are the base queries"""
    with np.errstate(over="ignore"):
        Q = (KM.queries(c, vs) * s).astype(np.float32)
    return np.concatenate([Q, extra_queries(vs, s)])


def answered(orc, Q, nbase, n, ef):
    """bool per query: the oracle answers it (the queries behind the base ones run alone: a batch raises as a whole)"""
    from oracle import oracle_py as O
    ok = np.ones(Q.shape[0], dtype=bool)
    for i in range(nbase, Q.shape[0]):
        try:
            orc.search_batch(Q[i:i + 1], max(n, 1), max(ef, 1))
        except O.OracleError as e:
            assert e.code == -2, e  # (NaN: Dist::cmp or partial_cmp().unwrap() panics in the reference)
            ok[i] = False
    return ok


# ---- the runner --------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def unchecked():
    """the return codes of the product calls made inside the block instead of exceptions (the arrays a failed batch
    call leaves are its per-query answer)"""
    from hnsw_rs_amd import hnsw as HH
    rcs, old = [], HH.check
    HH.check = rcs.append
    try:
        yield rcs
    finally:
        HH.check = old


def raises_nan(fn, what):
    import hnsw_rs_amd as H
    try:
        fn()
    except H.HnswError as e:
        assert e.code == H._lib.ERR_NAN_INPUT, (what, e)
        return
    raise AssertionError("%s: no error for a query the oracle refuses" % what)


def mixed_batch(c, idx, orc, rows, Q, ok, n, what):
    """the whole batch, raising queries included: an error status and count 0 exactly where the oracle raised, every
    other row the product's own answer without them (which KM.run_call has just held to the oracle)"""
    import hnsw_rs_amd as H
    from oracle import oracle_py as O
    NAN = H._lib.ERR_NAN_INPUT
    bad = np.nonzero(~ok)[0]
    if c.entry in ("batch", "filtered", "filtered_exact"):
        if c.entry == "batch":
            call = lambda QQ: idx.search_batch(QQ, n, c.ef)
        else:
            allow = np.random.default_rng(c.d * 31 + c.ef).random(N_POINTS) < 0.5  # (KM._calls' mask)
            idx.set_option("filter_exact_max", 10 ** 9 if c.entry == "filtered_exact" else -1)
            call = lambda QQ: idx.search_batch_filtered(QQ, n, c.ef, allow)
        with unchecked() as rcs:
            got = call(Q)
        clean = call(Q[ok])
        status = got[3][:, 3].astype(np.int32)
        assert rcs == [NAN if bad.size else 0], (what, rcs)
        assert np.array_equal(status != 0, ~ok) and (status[bad] == NAN).all(), (what, status, ok)
        assert (got[2][bad] == 0).all() and (got[0][bad] == O.UINT32_MAX).all(), (what, got[2][bad])
        for a, b in zip(got, clean):
            a, b = np.asarray(a)[ok], np.asarray(b)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b), what
    elif c.entry == "layer":
        ent = np.arange(c.ent, dtype=np.uint32) * 3 % N_POINTS
        for i in bad:
            raises_nan(lambda: idx.search_layer(0, Q[i], ent, c.ef), "%s query %d" % (what, i))
    elif c.entry == "brute":
        for i in bad:
            raises_nan(lambda: idx.brute_force(Q[i:i + 1], n), "%s query %d" % (what, i))
        if bad.size:
            raises_nan(lambda: idx.brute_force(Q, n), what)
    elif c.entry == "distance":
        # dist2many orders nothing: neither side raises on a NaN distance; NaN where the oracle has NaN, its bits elsewhere
        ids = np.arange(N_POINTS, dtype=np.uint32)
        for i in bad:
            g, w = idx.distance_batch(Q[i], ids), orc.distance_batch(Q[i], ids)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, i)
            assert np.array_equal(g[~np.isnan(w)].view(np.uint32), w[~np.isnan(w)].view(np.uint32)), (what, i)
    else:
        raise ValueError(c.entry)


def run_call(kernels, c, recipe):
    idx, orc, rows, s = fixture(c.kind, c.d, c.m, recipe)
    vs = KM.fixture(c.kind, c.d, c.m)[2]
    Q = queries(c, vs, s)
    ok = answered(orc, Q, c.nq, 10, c.ef)
    KM.run_call(kernels, c, on=(idx, orc, rows, Q[ok]))
    for n in sorted({10, c.n}) if c.entry != "distance" else (0,):
        mixed_batch(c, idx, orc, rows, Q, ok, n, "%s %s n=%d" % (recipe, KM.call_id(c), n))
    return int((~ok).sum())


# ---- brute_fast --------------------------------------------------------------------------------------------------------
FAST_KERNELS = {"hx_row_norms_kernel", "hx_brute_mfma_kernel", "hx_pair_distance_kernel"}
EXACT_KERNELS = {"hx_row_norms_kernel", "hx_brute_kernel<1>"}  # a call handed to the exact scan (after the norms)


def brute_fast_contract(idx, orc, X, Q, k, what, every=False):
    """both promises of brute_mfma.hip's header, whichever kernels served the call: on the queries that
    ground_truth_inputs.safe accepts the oracle's brute force bit for bit; on all others k distinct stored ids with the
    oracle's own distances of those ids in (dist, id) order (every: the oracle's answer on every query, as where the
    scores are exact).  -> the kernel log"""
    import hnsw_rs_amd as H
    from tests import ground_truth_inputs as G
    with H.kernel_log() as log:
        g_ids, g_d = idx.brute_force_fast(Q, k)
    w_ids, w_d = orc.brute_force(Q, k, nthreads=8)
    with np.errstate(all="ignore"):
        safe = G.safe(X, Q, k, w_ids)
    same = (g_ids == w_ids).all(axis=1) & (g_d.view(np.uint32) == w_d.view(np.uint32)).all(axis=1)
    assert same[safe | every].all(), (what, np.nonzero((safe | every) & ~same)[0])
    for qi in np.nonzero(~safe)[0]:
        i, dd = g_ids[qi], g_d[qi]
        assert (i < X.shape[0]).all() and len(set(i.tolist())) == len(i), (what, qi, i)
        assert np.array_equal(dd.view(np.uint32), orc.distance_batch(Q[qi], i).view(np.uint32)), (what, qi)
        keys = list(zip(dd.tolist(), i.tolist()))
        assert keys == sorted(keys), (what, qi, keys)
    return set(log)


def run_brute_fast(recipe):
    """the matrix's brute_fast call on the recipe's rows.  Every recipe leaves the range in which the screen's error
    bound means anything (rows below 2^-48 or above 2^40), so the call must be the exact scan's -- and the contract
    holds whether or not the matrix cores flush subnormals."""
    (kernels, c), = BRUTE_FAST
    idx, orc, rows, s = fixture(c.kind, c.d, c.m, recipe)
    Q = queries(c, KM.fixture(c.kind, c.d, c.m)[2], s)  # (f32: the oracle answers every one of them)
    log = brute_fast_contract(idx, orc, rows, Q, c.ef, "brute_fast %s" % recipe)
    assert log == EXACT_KERNELS, (recipe, log)


def main(group):
    env = KM.GROUPS[group]
    for k, v in env.items():
        assert os.environ.get(k) == v, "run group %s with %s=%s" % (group, k, v)
    calls = 0
    for recipe in (sys.argv[2:] or RECIPES):
        for kernels, c in TABLE:
            if c.group == group:
                run_call(kernels, c, recipe)
                calls += 1
    print("NUMERIC RANGE OK %s %d" % (group, calls))


if __name__ == "__main__":
    main(sys.argv[1])
