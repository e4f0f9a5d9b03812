"""hnsw_search_batch_filtered_wide on the MI355X, bit for bit: the graph path against the CPU restatement
(tests/filtered_restate.py) at n and ef' up to 1024 under every kind of filter, with the visited set mostly in LDS and
mostly in HBM; against hnsw_search_batch_filtered_set_range where both accept the shape; against the oracle's
ann_by_vector without a filter; the exact path at its segment edges; the overflow of both levels of the visited set."""
import ctypes as C

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests import filtered_restate as FR
from tests.test_gpu_filtered import restated
from tests.util import assert_search_equal, oracle_from_product, rand_vectors

pytestmark = pytest.mark.gpu

N, D, M, NQ = 6000, 24, 8, 8
NONE = _lib.MASK_NONE
HBM_LIMIT = 3 * (1 << 18) // 4  # ids the default HBM level holds
A_SIZES = (64, 1023, 2049, 5000)  # rows 1.. of the set: n - 1 for both n, two segments with one id in the second, three


class World:
    def __init__(self, kind):
        rng = np.random.default_rng(11)
        self.vs = rand_vectors(N, D, 7)
        self.vs[200:204] = self.vs[100:104]  # equal distances: ordered by id
        self.lv = O.draw_levels(N, M, 3)
        self.index = H.HNSW.new(M, 32, D, kind).insert_bulk(self.vs, 2, False, levels=self.lv)
        self.ridx = restated(self.index, self.vs)
        self.Q = rand_vectors(NQ, D, 8)
        self.Q[0] = self.vs[100]
        self.lab = rng.integers(0, 10, size=N).astype(np.uint32)
        self.deleted = rng.choice(N, 50, replace=False)
        self.alive = np.ones(N, dtype=bool)
        self.alive[self.deleted] = False
        self.rows = np.zeros((1 + len(A_SIZES), N), dtype=bool)
        self.rows[0] = rng.random(N) < 0.5
        for r, a in enumerate(A_SIZES):  # exactly a admissible ids each
            self.rows[1 + r, rng.choice(np.flatnonzero(self.alive), a, replace=False)] = True
        self.index.set_labels(self.lab)
        self.index.mark_deleted(self.deleted)
        self.set = self.index.mask_set(self.rows)

    def admissible(self, mo, lo, hi, qi):
        a = self.alive.copy()
        if mo is not None and mo[qi] != NONE:
            a &= self.rows[mo[qi]]
        if lo is not None:
            a &= (self.lab >= lo[qi]) & (self.lab <= hi[qi])
        return a

    def wide(self, Q, n, ef, mo=None, lo=None, hi=None):
        """the C entry itself -> status, (ids, dists, counts, stats, paths)"""
        nq = Q.shape[0]
        arr = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (mo, lo, hi)]
        ids = np.zeros((nq, n), dtype=np.uint32)
        dists = np.zeros((nq, n), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        stats = np.zeros((nq, 4), dtype=np.int32)
        paths = np.full(nq, 9, dtype=np.uint8)

        def p(a, t=C.c_uint32):
            return None if a is None else a.ctypes.data_as(C.POINTER(t))
        rc = _lib.lib().hnsw_search_batch_filtered_wide(
            self.index._h, p(np.ascontiguousarray(Q, dtype=np.float32), C.c_float), nq, n, ef,
            None if mo is None else self.set._s, *[p(x) for x in arr], p(ids), p(dists, C.c_float), p(counts),
            C.cast(stats.ctypes.data, C.POINTER(_lib.QueryStats)), p(paths, C.c_uint8))
        return rc, (ids, dists, counts, stats.astype(np.int64), paths)

    def options(self, exact_max, lds=0, hbm=18):
        self.index.set_option("filter_exact_max", exact_max)
        self.index.set_option("filter_wide_lds_log2", lds)
        self.index.set_option("filter_wide_hbm_log2", hbm)


@pytest.fixture(scope="module", params=[H.VEC_F32, H.VEC_QUANT8], ids=["f32", "quant8"])
def world(request):
    w = World(request.param)
    yield w
    w.set.close()


def u32(x):
    return np.full(NQ, x, dtype=np.uint32)


FILTERS = {
    "deleted": (None, None, None),
    "row": (u32(0), None, None),
    "range": (None, u32(3), u32(3)),
    "row and range": (u32(0), u32(2), u32(6)),
    "mixed": (np.array([0, NONE] * 4, dtype=np.uint32), np.array([0, 3, 5, 0, 4, 7, 2, 0], dtype=np.uint32),
              np.array([9, 3, 8, 0xFFFFFFFF, 1, 9, 2, 4], dtype=np.uint32)),  # query 4: an empty range
}


def equal_row(got, qi, want, n, what):
    w_ids, w_d, w_c = FR.padded(want, n)
    assert got[2][qi] == w_c, (what, qi)
    assert np.array_equal(got[0][qi], w_ids), (what, qi, got[0][qi][:8], w_ids[:8])
    assert np.array_equal(got[1][qi].view(np.uint32), w_d.view(np.uint32)), (what, qi)
    assert tuple(got[3][qi, :3]) == tuple(want["counters"]) and got[3][qi, 3] == 0, (what, qi, got[3][qi], want["counters"])


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("n,ef", [(65, 65), (200, 257), (10, 1024), (1024, 1024)])
def test_graph_path_equals_the_restatement(world, n, ef, filt):
    mo, lo, hi = FILTERS[filt]
    want = [FR.graph(world.ridx, world.Q[qi], n, ef, lambda i, a=world.admissible(mo, lo, hi, qi): bool(a[i]), order="batch")
            for qi in range(NQ)]
    for g in want:  # on the CPU: no query comes near the room of the smaller LDS level plus the HBM level
        assert g["visited0"] + g["maxdeg0"] <= 768 + HBM_LIMIT
    for lds in (0, 10):  # the launcher's LDS level; 768 ids in LDS and the rest through HBM
        world.options(-1, lds)
        with H.kernel_log() as log:
            rc, got = world.wide(world.Q, n, ef, mo, lo, hi)
        assert rc == 0 and (got[4] == 0).all(), (rc, got[4])
        assert dict(log) == {"hx_filt_wide_kernel<%d, 0, 0>" % world.index.vec_kind: 1}, dict(log)
        for qi in range(NQ):
            equal_row(got, qi, want[qi], n, (filt, "lds", lds))
    if filt == "mixed":
        assert got[2][4] == 0 and (got[0][4] == _lib.UINT32_MAX).all() and np.isinf(got[1][4]).all()
    assert not np.isin(got[0], world.deleted).any()


@pytest.mark.parametrize("exact_max", [-1, 65536])
@pytest.mark.parametrize("n,ef", [(10, 64), (64, 256)])
def test_equals_the_set_range_entry_point(world, n, ef, exact_max):
    mo, lo, hi = FILTERS["mixed"]
    world.options(exact_max)
    want = world.index.search_batch_filtered_set_range(world.Q, n, ef, world.set, mo.astype(np.int64), lo, hi)
    rc, got = world.wide(world.Q, n, ef, mo, lo, hi)
    assert rc == 0
    for k in range(5):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), k
    assert set(got[4].tolist()) == ({0} if exact_max < 0 else {1})


FORMS = {(H.VEC_F32, 100): "1, 25, 100", (H.VEC_F32, 128): "1, 32, 128", (H.VEC_QUANT8, 100): "0, 4, 100"}


@pytest.mark.parametrize("kind,d", list(FORMS))
def test_compiled_forms_equal_the_set_range_entry_point(kind, d):
    vs, qs = rand_vectors(3000, d, 40 + d), rand_vectors(NQ, d, 41 + d)
    index = H.HNSW.new(16, 64, d, kind).insert_bulk(vs, 4, False, levels=O.draw_levels(3000, 16, 2))
    rng = np.random.default_rng(d)
    index.set_labels(rng.integers(0, 5, size=3000).astype(np.uint32))
    s = index.mask_set([rng.random(3000) < 0.5])
    index.set_option("filter_exact_max", -1)
    index.set_option("filter_wide_lds_log2", 10)
    want = index.search_batch_filtered_set_range(qs, 64, 256, s, None, 1, 3)
    with H.kernel_log() as log:
        got = index.search_batch_filtered_wide(qs, 64, 256, s, None, 1, 3)
    assert dict(log) == {"hx_filt_wide_kernel<%s>" % FORMS[kind, d]: 1}, dict(log)
    for k in range(5):
        a, b = got[k], want[k]
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), k
    assert (got[4] == 0).all() and got[2].min() == 64
    s.close()


def test_unfiltered_equals_ann_by_vector(world):
    world.index.unmark_deleted(world.deleted)
    try:
        world.options(-1)
        rc, got = world.wide(world.Q, 300, 500)
        orc = oracle_from_product(world.index, world.vs, world.lv)
        assert rc == 0 and (got[4] == 0).all()
        assert_search_equal(got[:4], orc.search_batch(world.Q, 300, 500), "unfiltered")
    finally:
        world.index.mark_deleted(world.deleted)


@pytest.mark.parametrize("n", [65, 1024])
def test_exact_path_equals_the_restatement(world, n):
    Q = world.Q.copy()
    Q[5, 3] = np.nan
    mo = np.array([1 if n == 65 else 2, 3, 4, 3, 4, 4, 0, NONE], dtype=np.uint32)  # A = n - 1, 2049, 5000, ...
    world.options(10 ** 9)
    with H.kernel_log() as log:
        rc, got = world.wide(Q, n, n, mo)
    assert rc == _lib.ERR_NAN_INPUT and (got[4] == 1).all()
    # five groups: a compaction, a scan and a merge each
    assert dict(log) == {"hx_filt_compact_kernel": 5, "hx_filt_wide_scan_kernel<%d>" % world.index.vec_kind: 5,
                         "hx_filt_wide_merge_kernel": 5}, dict(log)
    for qi in range(NQ):
        if qi == 5:
            assert got[3][qi, 3] == _lib.ERR_NAN_INPUT and got[2][qi] == 0 and (got[0][qi] == _lib.UINT32_MAX).all()
            continue
        a = np.flatnonzero(world.admissible(mo, None, None, qi))
        assert qi > 2 or a.size == (n - 1, 2049, 5000)[qi]
        equal_row(got, qi, FR.exact(world.ridx, Q[qi], n, a), n, ("exact", n))


def test_a_full_visited_set_is_answered_by_the_exact_path(world):
    _, lo, hi = FILTERS["range"]
    limit = 768 + 768
    world.options(-1, 10, 10)
    before = [world.index.stat("filtered_wide_" + k) for k in ("overflow_exact", "queries_graph")]
    rc, got = world.wide(world.Q, 200, 1024, None, lo, hi)
    assert rc == 0
    n2 = 0
    for qi in range(NQ):
        adm = world.admissible(None, lo, hi, qi)
        g = FR.graph(world.ridx, world.Q[qi], 200, 1024, lambda i: bool(adm[i]), order="batch")
        if g["visited0"] > limit:
            assert got[4][qi] == 2, (qi, g["visited0"])
        if g["visited0"] + g["maxdeg0"] <= limit:
            assert got[4][qi] == 0, (qi, g["visited0"])
        n2 += int(got[4][qi] == 2)
        equal_row(got, qi, g if got[4][qi] == 0 else FR.exact(world.ridx, world.Q[qi], 200, np.flatnonzero(adm)), 200, "overflow")
    assert n2 > 0
    after = [world.index.stat("filtered_wide_" + k) for k in ("overflow_exact", "queries_graph")]
    assert after[0] - before[0] == n2 and after[1] - before[1] == NQ - n2
