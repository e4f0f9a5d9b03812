"""hnsw_search_batch_filtered_wide without a GPU: the limits are refused before the device is touched, the two options
take their ranges only, the four counters exist, the kernels use no scratch, and every kernel of the wide library
(libhnsw_mi355x_wide.so, beside the main one) is named here with the GPU test that asserts with the launch log that it ran."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from oracle import oracle_py as O
from tests.kernel_resources import resource_usage
from tests.util import rand_vectors

NQ, D = 3, 8


@pytest.fixture(scope="module")
def index():
    vs = rand_vectors(300, D, 1)
    return H.HNSW.new(8, 32, D).insert_bulk(vs, 1, False, levels=O.draw_levels(300, 8, 1))


def call(index, n, ef, lo=None, hi=None):
    def p(a, t=C.c_uint32):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))
    Q = rand_vectors(NQ, D, 2)
    ids = np.zeros((NQ, max(n, 1)), dtype=np.uint32)
    return _lib.lib().hnsw_search_batch_filtered_wide(index._h, p(Q, C.c_float), NQ, n, ef, None, None, p(lo), p(hi), p(ids),
                                                      None, None, None, None)


@pytest.mark.parametrize("n,ef,ranged", [(0, 64, ""), (1025, 64, ""), (10, 1025, ""), (1025, 1025, ""), (10, 64, "lo"),
                                         (10, 64, "hi")])
def test_outside_the_limits_is_an_argument_error(index, n, ef, ranged):
    r = np.zeros(NQ, dtype=np.uint32)
    assert call(index, n, ef, r if ranged == "lo" else None, r if ranged == "hi" else None) == _lib.ERR_ARG
    assert index.stat("uploads") == 0  # (decided before any GPU work)


@pytest.mark.parametrize("name,good,bad", [("filter_wide_lds_log2", (0, 10, 15), (-1, 9, 16)),
                                           ("filter_wide_hbm_log2", (0, 10, 18, 22), (-1, 9, 23))])
def test_options_take_their_ranges_only(index, name, good, bad):
    for v in good:
        index.set_option(name, v)
    for v in bad:
        with pytest.raises(H.HnswError) as e:
            index.set_option(name, v)
        assert e.value.code == _lib.ERR_ARG, (name, v)


def test_the_counters_exist_and_start_at_zero(index):
    for name in ("filtered_wide_calls", "filtered_wide_queries_graph", "filtered_wide_queries_exact",
                 "filtered_wide_overflow_exact"):
        assert index.stat(name) == 0, name


@pytest.mark.skipif(not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_wide_kernels_have_no_scratch_or_spills():
    """search_filtered_wide.hip compiled for gfx950 with the Makefile's flags: five forms of the graph kernel, the scan
    for both kinds and the merge, none with scratch or spilled vector registers"""
    _, stderr = resource_usage("search_filtered_wide.hip", ("-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"))
    blocks = re.split(r"Function Name: ", stderr)[1:]
    assert sum("hx_filt_wide_kernel" in b for b in blocks) == 5 and len(blocks) == 8, [b.split()[0] for b in blocks]
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b
        assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b


# every __global__ instantiation of the wide library and the case of tests/test_gpu_filtered_wide.py that holds it to its
# reference and asserts with the kernel launch log that it ran
WIDE_KERNELS = {
    "hx_filt_wide_kernel<0, 0, 0>": "test_graph_path_equals_the_restatement[quant8-*]",
    "hx_filt_wide_kernel<1, 0, 0>": "test_graph_path_equals_the_restatement[f32-*]",
    "hx_filt_wide_kernel<0, 4, 100>": "test_compiled_forms_equal_the_set_range_entry_point[0-100]",
    "hx_filt_wide_kernel<1, 25, 100>": "test_compiled_forms_equal_the_set_range_entry_point[1-100]",
    "hx_filt_wide_kernel<1, 32, 128>": "test_compiled_forms_equal_the_set_range_entry_point[1-128]",
    "hx_filt_wide_scan_kernel<0>": "test_exact_path_equals_the_restatement[quant8-*]",
    "hx_filt_wide_scan_kernel<1>": "test_exact_path_equals_the_restatement[f32-*]",
    "hx_filt_wide_merge_kernel": "test_exact_path_equals_the_restatement",
}


def test_every_kernel_of_the_wide_library_has_a_parity_case():
    _lib.lib()
    blob = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "libhnsw_mi355x_wide.so"), "rb").read()
    compiled = {H.kernel_name(m.group(1).decode()) for m in re.finditer(rb"(_Z[A-Za-z0-9_]+)\.kd\x00", blob)}
    assert compiled == set(WIDE_KERNELS), sorted(compiled ^ set(WIDE_KERNELS))
