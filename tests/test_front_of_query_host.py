"""No GPU: the fixtures of tests/front_of_query.py do what their names promise on the oracle's own search_layer (the
top row's degree, the winner of the walk, the expansions a duplicate of the entry point's row causes, the ids that
share a home bucket of the upper layers' visited table, the quarters of the layer-0 table a first pass touches), and
the reference panics for every query of the two NaN cases: a fixture that stops provoking its path fails here."""
import numpy as np
import pytest

from tests import front_of_query as FQ


@pytest.mark.parametrize("name", sorted(FQ.CASES))
def test_case_has_its_pattern(name):
    FQ.assert_pattern(name)
    c, _ = FQ.fixture(name)
    assert len(c.queries) <= 16


@pytest.mark.parametrize("name", sorted(FQ.NAN_CASES))
def test_reference_panics(name):
    FQ.assert_panics(name)


def test_product_import_refuses_a_nan_in_a_stored_row():
    """why the NaN cases reach their NaN distance through + infinity: no product index holds a NaN row"""
    import hnsw_rs_amd as H
    c, _ = FQ.fixture("nan_entry")
    rows = c.rows.copy()
    rows[c.nan_row, 7] = np.nan
    idx = H.HNSW.new(FQ.M, 32, FQ.D, FQ.UW.F32)
    with pytest.raises(H.HnswError) as e:
        idx.import_points(rows, c.levels)
    assert e.value.code == H._lib.ERR_NAN_INPUT
    FQ.product("nan_entry")  # the case as laid: taken


def test_home_is_the_kernels_hash():
    """Visited::home by hand for three ids: (id * 0x9E3779B1 mod 2^32) >> (32 - log2(buckets))"""
    assert [int(x) for x in FQ.home([0, 1, 2], 10)] == [0, 0x9E3779B1 >> 24, (2 * 0x9E3779B1 & 0xFFFFFFFF) >> 24]
    assert FQ.home_upper(np.arange(FQ.N)).max() < 256 and FQ.quarter_layer0(np.arange(FQ.N)).max() == 3
