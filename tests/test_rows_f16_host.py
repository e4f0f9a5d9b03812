"""The option "rows_f16" on the host: an index under it over X IS the plain f32 index over
X.astype(float16).astype(float32); what the option refuses; the default-deny guard.  No GPU: the guard sits before any
device call."""
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.util import oracle_from_product, rand_vectors, same_graph

N, D, M = 400, 24, 8


def f16_index(d=D, kind=H.VEC_F32):
    idx = H.HNSW.new(M, 32, d, kind)
    idx.set_option("rows_f16", 1)
    return idx


def refused(code, call, *args):
    with pytest.raises(H.HnswError) as e:
        call(*args)
    assert e.value.code == code, e.value
    return str(e.value)


@pytest.fixture(scope="module")
def rows():
    X = rand_vectors(N, D, 11) * 2 - 0.5
    X[0, :4] = [1 + 2.0**-11, 1 + 3 * 2.0**-11, -(1 + 2.0**-11), 2.0**-25]  # exact ties between two f16 values
    X[1] *= np.float32(2.0**-18)                                            # f16 subnormals
    X[2, :2] = [65504.0, -65504.0]
    X[3, 0] = 65519.0                                                       # the last value below the tie to inf
    return X, X.astype(np.float16).astype(np.float32), O.draw_levels(N, M, 5)


def test_is_the_plain_index_over_the_rounded_rows(rows, tmp_path):
    X, X16, lv = rows
    assert np.array_equal(X16[0, :4], np.float32([1, 1 + 2.0**-9, -1, 0])) and X16[3, 0] == 65504
    a = f16_index().insert_bulk(X, 1, False, levels=lv)
    b = H.HNSW.new(M, 32, D, H.VEC_F32).insert_bulk(X16, 1, False, levels=lv)
    a.save(tmp_path / "a"), b.save(tmp_path / "b")
    files = [{str(p.relative_to(tmp_path / s)): p.read_bytes() for p in (tmp_path / s).rglob("*") if p.is_file()} for s in "ab"]
    assert files[0] and files[0] == files[1]
    assert same_graph(a, oracle_from_product(b, X16, lv))
    assert same_graph(a.clone(), oracle_from_product(b, X16, lv))
    # ... and so is one grown a point at a time, a clone keeping the option
    c = f16_index().insert_bulk(X[:N - 3], 1, False, levels=lv[:N - 3]).clone()
    d = H.HNSW.new(M, 32, D, H.VEC_F32).insert_bulk(X16[:N - 3], 1, False, levels=lv[:N - 3])
    for i in range(N - 3, N):
        c.insert_vec(X[i], int(lv[i])), d.insert_vec(X16[i], int(lv[i]))
    assert same_graph(c, oracle_from_product(d, X16, lv))
    # a loaded index whose rows are f16 values takes the option: the file has no field for it
    H.HNSW.load(tmp_path / "a").set_option("rows_f16", 1)


def test_option_refusals(rows):
    X, _, lv = rows
    refused(_lib.ERR_ARG, f16_index, D, H.VEC_QUANT8)
    plain = H.HNSW.new(M, 32, D, H.VEC_F32).insert_bulk(X[:50], 1, False, levels=lv[:50])  # 0.1-like values stored
    assert "binary16" in refused(_lib.ERR_ARG, plain.set_option, "rows_f16", 1)
    refused(_lib.ERR_ARG, plain.set_option, "rows_f16", 2)


@pytest.mark.parametrize("value,code", [(65520.0, _lib.ERR_ARG), (-np.inf, _lib.ERR_ARG), (np.nan, _lib.ERR_NAN_INPUT)])
def test_input_errors(rows, value, code):
    X = rows[0][:8].copy()
    X[5, 3] = value
    idx = f16_index()
    refused(code, idx.insert_bulk, X, 1, False)
    refused(code, idx.insert_vec, X[5])
    assert len(idx) == 0


def test_every_kernel_of_the_rows16_library_has_a_parity_case():
    """libhnsw_mi355x_rows16.so holds hx_search16_kernel<DS, R> for the four row forms x the list widths the launcher
    picks; tests/test_gpu_rows_f16.py (kernel_for, test_every_dimension_path, test_every_list_width_of_every_gather,
    test_list_widths) asserts with the launch log that each ran and holds its answers to the oracle"""
    _lib.lib()
    blob = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "libhnsw_mi355x_rows16.so"), "rb").read()
    compiled = {H.kernel_name(m.group(1).decode()) for m in re.finditer(rb"(_Z[A-Za-z0-9_]+)\.kd\x00", blob)}
    want = {"hx_search16_kernel<%d, %d>" % (ds, r) for ds in (0, 128, 256, 768) for r in (1, 2, 4, 8)}
    assert compiled == want | {"hx_search16_kernel<0, 16>"}, sorted(compiled ^ want)


def test_unserved_entry_points_refuse_instead_of_answering(rows):
    X, _, lv = rows
    idx = f16_index().insert_bulk(X, 1, False, levels=lv)
    Q = X[:4]
    for call, args in [(idx.search_batch_filtered, (Q, 5, 32, np.arange(100))), (idx.brute_force, (Q, 5)),
                       (idx.search_layer, (0, Q[0], [0], 8))]:
        assert "rows_f16" in refused(_lib.ERR_ARG, call, *args)
