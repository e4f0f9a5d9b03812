"""One filter through every family of filtered search on the MI355X.  The families share one host path ("The
filter of a call"), so what no per-family file looks for is cross-talk between them: "label in {2, 5}" over labels
id % 7 is stated as a packed mask, as a _multi call whose queries all name row 0, as row 0 of a resident set, as that
row AND [0, UINT32_MAX], as HNSW_MASK_NONE AND one range (over a second label assignment under which the set is the
range [2, 3]), as a list of two ranges, as a padded list of four with a duplicate, and, over the second assignment, as
the range call and as a list of one.  Every form gives the same ids, distance bits, counts and paths, on the graph
path (filter_exact_max = -1) and on the exact path; around each call exactly its own family's counters move; a graph
call is one launch of the graph kernel.  The four device-pointer forms against the host form.  (Path 2 needs more than
24576 admissible ids: the three_paths fixtures of the per-family files cover it.)"""

import numpy as np
import pytest

import hnsw_rs_amd as H
from oracle import oracle_py as O
from tests import test_gpu_filtered_ranges as TR
from tests import test_gpu_filtered_set_range as TSR
from tests import test_gpu_labels as TL
from tests import test_gpu_mask_set as TS
from tests.test_gpu_filtered_multi import graph_kernels
from tests.test_gpu_mask_set import delta, stats_of
from tests.util import rand_vectors

pytestmark = pytest.mark.gpu

N, D, M, NQ, TOP, EF = 3001, 12, 8, 64, 5, 32
MAX = 0xFFFFFFFF
FAMILY = {  # the counters of a family, and what one call under one filter adds to them
    "mask": {},
    "multi": {"filtered_multi_calls": 1, "filtered_multi_masks": 1},
    "set": {"filtered_set_calls": 1},
    "range": {"filtered_range_calls": 1, "filtered_range_ranges": 1},
    "set_range": {"filtered_set_range_calls": 1, "filtered_set_range_groups": 1},
    "ranges": {"filtered_ranges_calls": 1, "filtered_ranges_groups": 1},
}
PATHS = ("filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact", "deleted_queries_graph",
         "deleted_queries_exact", "deleted_overflow_exact")
KEYS = tuple(k for f in FAMILY.values() for k in f) + PATHS
LABELS_A = (np.arange(N) % 7).astype(np.uint32)              # the set: labels 2 and 5
LABELS_B = np.array([0, 1, 2, 4, 5, 3, 6], dtype=np.uint32)[LABELS_A]  # 2 -> 2, 5 -> 3: the set is [2, 3]
MASK = (LABELS_A == 2) | (LABELS_A == 5)
ROW0, NONE = np.zeros(NQ, dtype=np.int64), np.full(NQ, -1, dtype=np.int64)


@pytest.fixture(scope="module", params=[H.VEC_QUANT8, H.VEC_F32], ids=["quant8", "f32"])
def world(request):
    vs = rand_vectors(N, D, 61)
    index = H.HNSW.new(M, 32, D, request.param).insert_bulk(vs, 2, False, levels=O.draw_levels(N, M, 61))
    return index, index.mask_set([MASK]), rand_vectors(NQ, D, 62)


def host_forms(index, s, Q):
    """(name, family, labels, the call) of every host form of the filter"""
    i = index
    return (
        ("mask", "mask", LABELS_A, lambda: i.search_batch_filtered(Q, TOP, EF, MASK)),
        ("multi, row 0", "multi", LABELS_A, lambda: i.search_batch_filtered_multi(Q, TOP, EF, [MASK], ROW0)),
        ("set, row 0", "set", LABELS_A, lambda: i.search_batch_filtered_set(Q, TOP, EF, s, ROW0)),
        ("set row AND every label", "set_range", LABELS_A, lambda: i.search_batch_filtered_set_range(Q, TOP, EF, s, ROW0, 0, MAX)),
        ("no row AND [2, 3]", "set_range", LABELS_B, lambda: i.search_batch_filtered_set_range(Q, TOP, EF, s, NONE, 2, 3)),
        ("ranges, K = 2", "ranges", LABELS_A, lambda: i.search_batch_filtered_ranges(Q, TOP, EF, [[2, 5]] * NQ)),
        ("ranges, K = 4", "ranges", LABELS_A,
         lambda: i.search_batch_filtered_ranges(Q, TOP, EF, [[5, (1, 0), (2, 2), (5, 5)]] * NQ)),
        ("range [2, 3]", "range", LABELS_B, lambda: i.search_batch_filtered_range(Q, TOP, EF, 2, 3)),
        ("ranges, K = 1", "ranges", LABELS_B, lambda: i.search_batch_filtered_ranges(Q, TOP, EF, [[(2, 3)]] * NQ)),
    )


def same(a, b, what):
    """two results: ids, distance bits, counts and paths equal bit for bit"""
    for name, k in (("ids", 0), ("dists", 1), ("counts", 2), ("paths", 4)):
        x, y = (np.ascontiguousarray(r[k]) for r in (a, b))
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:5])


def moved(family, graph, exact):
    want = dict.fromkeys(KEYS, 0)
    want.update(FAMILY[family])
    want["filtered_queries_graph"], want["filtered_queries_exact"] = graph, exact
    return want


@pytest.mark.parametrize("exact_max", [-1, 1 << 20], ids=["graph", "exact"])
def test_every_host_form_of_one_filter_gives_one_answer_and_counts_as_its_own_family(world, exact_max):
    index, s, Q = world
    index.set_option("filter_exact_max", exact_max)
    graph = exact_max < 0
    first = None
    for name, family, labels, call in host_forms(index, s, Q):
        index.set_labels(labels)
        before = stats_of(index, KEYS)
        with H.kernel_log() as log:
            got = call()
        assert delta(index, before) == moved(family, NQ if graph else 0, 0 if graph else NQ), name
        assert sum(graph_kernels(log).values()) == (1 if graph else 0), (name, log)
        assert (got[4] == (0 if graph else 1)).all() and (got[3][:, 3] == 0).all(), name
        assert all(MASK[got[0][q, : got[2][q]]].all() for q in range(NQ)), name
        if first is None:
            first = got
        same(got, first, name)


def test_every_device_form_equals_its_host_form_and_counts_as_its_own_family(world):
    index, s, Q = world
    index.set_option("filter_exact_max", -1)
    lo, hi = np.full(NQ, 2, dtype=np.uint32), np.full(NQ, 3, dtype=np.uint32)
    forms = (
        ("set", "set", LABELS_A, lambda: index.search_batch_filtered_set(Q, TOP, EF, s, ROW0),
         lambda log: TS.device_call(index, s, Q, TOP, EF, ROW0, log_enqueue=log)),
        ("range", "range", LABELS_B, lambda: index.search_batch_filtered_range(Q, TOP, EF, lo, hi),
         lambda log: TL.device_call(index, Q, TOP, EF, lo, hi, log_enqueue=log)),
        ("set_range", "set_range", LABELS_B, lambda: index.search_batch_filtered_set_range(Q, TOP, EF, s, NONE, lo, hi),
         lambda log: TSR.device_call(index, s, Q, TOP, EF, NONE, lo, hi, log_enqueue=log)),
        ("ranges", "ranges", LABELS_A, lambda: index.search_batch_filtered_ranges(Q, TOP, EF, [[2, 5]] * NQ),
         lambda log: TR.device_call(index, Q, TOP, EF, [[2, 5]] * NQ, log_enqueue=log)),
    )
    first = None
    for name, family, labels, host, device in forms:
        index.set_labels(labels)
        want = host()
        before = stats_of(index, KEYS)
        log = {}
        code, got = device(log)
        assert code is None, name
        assert delta(index, before) == moved(family, NQ, 0), name
        assert sum(graph_kernels(log).values()) == 1, (name, log)
        same(got, want, name)
        if first is None:
            first = got
        same(got, first, name)
