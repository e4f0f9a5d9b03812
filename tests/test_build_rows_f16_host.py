"""The on-device build under "rows_f16" on the host: the kernel set of libhnsw_mi355x_build16.so, and
the threaded rounding pass every bulk insert goes through.  No GPU."""
import os
import re

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.test_gpu_build_rows_f16 import CASES


def test_every_kernel_of_the_build16_library_has_a_parity_case():
    _lib.lib()
    blob = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "libhnsw_mi355x_build16.so"), "rb").read()
    compiled = {H.kernel_name(m.group(1).decode()) for m in re.finditer(rb"(_Z[A-Za-z0-9_]+)\.kd\x00", blob)}
    named = {"hx_insert16_kernel<%d>" % c[4] for c in CASES} | {"hx_connect16_kernel<%d>" % c[5] for c in CASES}
    assert len(named) == 7 and compiled == named, sorted(compiled ^ named)


N, D, M = 8 * 4096, 3, 4  # eight threads take 4096 rows each


def f16_index():
    idx = H.HNSW.new(M, 8, D, H.VEC_F32)
    idx.set_option("rows_f16", 1)
    return idx


@pytest.fixture(scope="module")
def rows():
    X = np.random.Generator(np.random.PCG64(16)).standard_normal((N, D), dtype=np.float32) * np.float32(100)
    X[7, 1], X[N - 9, 2] = 1 + 2.0**-11, 2.0**-25  # a tie between two f16 values, a value below the smallest subnormal
    return X, O.draw_levels(N, M, 7)


def test_the_rounding_pass_stores_the_same_bytes_on_1_and_8_threads(rows, tmp_path):
    X, lv = rows
    for t in (1, 8):  # (the graph of a racing 8-thread CPU build is its own: the points file holds the rows)
        f16_index().insert_bulk(X, t, False, levels=lv).save(tmp_path / str(t))
    assert (tmp_path / "1" / "points").read_bytes() == (tmp_path / "8" / "points").read_bytes()
    want = H.HNSW.new(M, 8, D, H.VEC_F32).insert_bulk(X.astype(np.float16).astype(np.float32), 1, False, levels=lv)
    want.save(tmp_path / "w")
    assert (tmp_path / "1" / "points").read_bytes() == (tmp_path / "w" / "points").read_bytes()


def test_the_refusal_names_the_lowest_row_whatever_the_thread_count(rows):
    X = rows[0].copy()
    X[N - 100, 0], X[5000, 2], X[5000, 1] = -70000.0, 65520.0, 1e9  # in the last thread's share and in the second's
    said = []
    for t in (1, 8):
        idx = f16_index()
        with pytest.raises(H.HnswError) as e:
            idx.insert_bulk(X, t, False)
        assert e.value.code == _lib.ERR_ARG and len(idx) == 0
        said.append(str(e.value))
    assert said[0] == said[1] and "row 5000 holds 1e+09" in said[0], said
