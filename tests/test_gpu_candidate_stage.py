"""The candidate stage the composite searches share (csrc/lists_host.h), at the places where grouped, diversified and
from-rows search moved onto it: they upload the queries once, make the cosine option's unit-length copy in place once and
run the search and its re-run loop themselves.  Every comparison is exact: ids, distance BITS, counts and statuses.
  1. a query that fills the first launch's visited table is run again from there, as often and by the same kernels as
     the plain search runs it again (the hand-made graph of tests/test_gpu_visited_limit.py);
  2. under the cosine option one call launches the normalisation once;
  3. grouped search under the cosine option is the collapse of search_batch's lists;
  4. while ids are deleted the candidates stay the host form's, and the rows composed on the device reach it as they
     were composed: normalised once, by the host form itself."""
import numpy as np
import pytest

import hnsw_rs_amd as H
from tests import diverse_cases as DC
from tests import from_rows_cases as FC
from tests import grouped_cases as GC
from tests.test_gpu_diverse import search_world
from tests.test_gpu_visited_limit import _graph

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
MERGE_KERNEL, NORMALISE_KERNEL = "hx_filt_merge_kernel", "hx_normalise_rows_kernel"
LAM = 0.5


def distance_kernel(index):
    return "hx_distance_kernel<%d>" % index.vec_kind


# ---- 1. the re-run loop at its new site ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", ["f32", "q8"])
def test_an_overflowed_query_is_run_again_as_the_plain_search_runs_it(kind_name):
    kind = {"f32": H.VEC_F32, "q8": H.VEC_QUANT8}[kind_name]
    idx, orc, q = _graph(kind, 3080)  # query 0 visits 3 081 ids on layer 0: more than a 2^12-slot table takes
    pool, ef = 16, 64
    idx.search_batch_diverse(q, 5, pool, ef, LAM)  # (the snapshot and the label column are in HBM from here on)
    idx.search_batch_grouped(q, 4, 2, pool, ef)
    with H.kernel_log() as plain:
        cand = idx.search_batch(q, pool, ef)
    assert sum(plain.values()) > 1, "the case is there for a re-run: %s" % dict(plain)
    assert (np.asarray(cand[3])[:, 3] == 0).all()

    with H.kernel_log() as log:
        got = idx.search_batch_diverse(q, 5, pool, ef, LAM)
    k = distance_kernel(idx)
    assert log.get(k) == 1 and k not in plain, (dict(log), dict(plain))
    assert {name: n for name, n in log.items() if name != k} == dict(plain), (dict(log), dict(plain))
    DC.assert_diverse_equal(got, H.mmr_select(cand[0], cand[1], cand[2], None, orc.distance, LAM, 5), "diverse " + kind_name)
    assert np.array_equal(got[4], cand[3]) and (got[4][:, 3] == 0).all()

    with H.kernel_log() as log:
        got = idx.search_batch_grouped(q, 4, 2, pool, ef)
    assert log.get(MERGE_KERNEL) == 1 and MERGE_KERNEL not in plain, (dict(log), dict(plain))
    assert {name: n for name, n in log.items() if name != MERGE_KERNEL} == dict(plain), (dict(log), dict(plain))
    want = H.group_by_label(cand[0], cand[1], cand[2], None, 4, 2)  # no label was set: every label 0, one group
    GC.assert_grouped_equal(got, want, "grouped " + kind_name)
    assert (got[4] == (np.asarray(cand[2]) > 0)).all() and (got[2] == 0).all()
    assert np.array_equal(got[5], cand[3]) and (got[5][:, 3] == 0).all()


# ---- 2 .. 4. the cosine option -------------------------------------------------------------------------------------------
N_OUT, POOL, EF, G, P, TOPN = 10, 64, 128, 8, 3, 10


@pytest.fixture(params=["f32-16", "quant8-16"])
def cosine_world(request):
    """tests/test_gpu_diverse.py's clustered index with the cosine option switched on over its rows as they are stored
    (the option normalises what arrives from then on: here, the queries), and switched off again afterwards"""
    index, orc, Q, _, _ = search_world(request.param)
    sources = np.arange(0, index.len(), 47, dtype=np.uint32)
    index.set_option("metric_cosine", 1)
    try:
        index.search_batch(Q, POOL, EF)  # (the snapshot is in HBM from here on)
        yield index, orc, Q, sources
    finally:
        index.set_option("metric_cosine", 0)


def test_the_unit_copy_is_made_once_per_call(cosine_world):
    index, _, Q, sources = cosine_world
    calls = {"diverse": lambda: index.search_batch_diverse(Q, N_OUT, POOL, EF, LAM),
             "grouped": lambda: index.search_batch_grouped(Q, G, P, POOL, EF),
             "by id": lambda: index.search_batch_by_id(sources, TOPN, EF)}
    for what, call in calls.items():
        call()  # (warm: the label column is in HBM)
        with H.kernel_log() as log:
            call()
        assert log.get(NORMALISE_KERNEL) == 1, (what, dict(log))


def test_grouped_under_the_cosine_option_is_the_collapse_of_search_batch(cosine_world):
    index, _, Q, _ = cosine_world
    labels = (np.arange(index.len()) % 7).astype(np.uint32)  # (search_world's column)
    with H.kernel_log() as log:
        cand = index.search_batch(Q, POOL, EF)
    assert NORMALISE_KERNEL in log, dict(log)
    got = index.search_batch_grouped(Q, G, P, POOL, EF)
    GC.assert_grouped_equal(got, H.group_by_label(cand[0], cand[1], cand[2], labels, G, P), "cosine")
    assert np.array_equal(got[5], cand[3]) and (got[5][:, 3] == 0).all()
    assert (got[4] >= 1).all() and (got[3] == P).any()


def test_deleted_ids_still_take_the_host_form_under_the_cosine_option(cosine_world):
    index, orc, Q, sources = cosine_world
    stored = np.stack([orc.get_vals(int(i)) for i in sources]).astype(np.float32)  # the rows as composed: not unit length
    near = np.asarray(index.search_batch(Q, 8, 64)[0])
    deleted = np.unique(np.concatenate([near[:12, 1], near[12:24, 3], sources[5:9]]))  # hits, and four of the sources
    index.mark_deleted(deleted)
    try:
        c = index.search_batch(Q, POOL, 64)
        got = index.search_batch_diverse(Q, N_OUT, POOL, 64, LAM)
        DC.assert_diverse_equal(got, H.mmr_select(c[0], c[1], c[2], None, orc.distance, LAM, N_OUT), "diverse, deleted")
        assert np.array_equal(got[4], c[3]) and not np.isin(got[0][got[0] != MAX], deleted).any()
        # search_batch normalises the composed rows itself, once: rows that reached it at unit length already would have
        # been normalised twice, which rounds differently
        c = index.search_batch(stored, TOPN + 1, 64)
        want = H.drop_ids(c[0], c[1], c[2], c[3][:, 3], sources.reshape(-1, 1), TOPN)
        got = index.search_batch_by_id(sources, TOPN, 64)
        FC.assert_drop_equal(got[:3], want, "by id, deleted")
        assert np.array_equal(got[3], c[3]) and not np.isin(got[0][got[0] != MAX], deleted).any()
    finally:
        index.unmark_deleted(deleted)
