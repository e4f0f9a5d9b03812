"""Every __global__ instantiation compiled into libhnsw_mi355x.so has a parity case (no GPU needed).  The names are
read off the library's gfx950 code objects (their `<mangled name>.kd` kernel descriptors) and normalised by
hnsw_kernel_name, the function the kernel launch log uses.  Each must be named by exactly one of: a row of the search
matrix (tests/kernel_matrix.py, run by tests/test_gpu_kernel_matrix.py), a case of
tests/test_gpu_build_restatement.py, or ELSEWHERE (a test that asserts with the log that it ran) / UNREACHABLE below
with a reason.  A new template, or a new
dispatch branch that instantiates one, without a parity case fails here."""
import os
import re

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib
from tests import kernel_matrix as KM
from tests.test_gpu_build_restatement import BUILD_KERNELS

# launched by entry points whose own tests assert with the kernel log that they ran, and hold the result to the
# reference; not part of the search matrix
ELSEWHERE = {
    "hx_deleted_scatter_kernel": "deletion's mask upload: test_gpu_deleted.py::test_search_batch_under_deletions",
    "hx_normalise_rows_kernel": "the metric_cosine option's query copy: test_gpu_configs.py::test_cosine_option_is_l2_on_unit_vectors",
    "hx_patch_kernel": "insert_vec's live snapshot patch: test_gpu_snapshot.py::test_a_patched_snapshot_stays_canonical",
    "hx_fat_rebuild_kernel": "insert_vec's inline-row patch: test_gpu_snapshot.py::test_a_patched_snapshot_stays_canonical",
    "hx_sort_rows_kernel": "the snapshot a device build keeps: test_gpu_snapshot.py::test_the_snapshot_a_device_build_leaves_is_the_restatement_byte_for_byte",
    "hx_pack_rows_kernel": "sharded build, row ownership: test_gpu_parity.py::test_sharded_device_build_two_ranks",
    "hx_apply_rows_kernel": "sharded build, row ownership: test_gpu_parity.py::test_sharded_device_build_two_ranks",
    "hx_filter_records_kernel": "sharded build, record exchange: test_gpu_parity.py::test_sharded_device_build_two_ranks",
    "hx_scatter_rows_kernel": "host-connect device build (gpu_build 1): test_gpu_parity.py::test_device_build_makes_a_valid_graph",
}
# compiled but never selected by any input
UNREACHABLE = {}
# rocPRIM's radix sort (build_sort.hip) instantiates its own kernels; rocPRIM launches them, not a launch site of
# ours, so the log cannot name them: the device build's sort is checked by the build restatement
LIBRARY_PREFIXES = ("rocprim::",)

LIB = _lib.LIB_PATH  # (the library hnsw_kernel_name comes from)


def compiled_kernels():
    """normalised names of the kernel descriptors in the library's (uncompressed) gfx950 code objects"""
    blob = open(LIB, "rb").read()
    mangled = set(m.group(1).decode() for m in re.finditer(rb"(_Z[A-Za-z0-9_]+)\.kd\x00", blob))
    assert mangled, "no kernel descriptors found in %s (compressed code objects?)" % LIB
    return {H.kernel_name(x) for x in mangled}


def matrix_kernels():
    return {k for row in KM.CASES for k in row.kernels}


def test_the_name_function_is_the_logs():
    _lib.lib()
    assert H.kernel_name("_ZN2hx16hx_search_kernelILi1ELi64ELi256ELi4ELb0EEEvNS_7DevViewENS_10SearchArgsEj") == \
        "hx_search_kernel<1, 64, 256, 4, false>"
    assert H.kernel_name("hx_patch_kernel") == "hx_patch_kernel"


def test_every_instantiation_has_exactly_one_home():
    compiled = {k for k in compiled_kernels() if not k.startswith(LIBRARY_PREFIXES)}
    homes = {"matrix": matrix_kernels(), "build restatement": set(BUILD_KERNELS), "ELSEWHERE": set(ELSEWHERE),
             "UNREACHABLE": set(UNREACHABLE)}
    missing = sorted(k for k in compiled if not any(k in h for h in homes.values()))
    assert not missing, "instantiations without a parity case: %s" % missing
    twice = sorted(k for k in compiled if sum(k in h for h in homes.values()) > 1)
    assert not twice, "instantiations listed in more than one place: %s" % twice


def test_no_case_names_an_instantiation_that_does_not_exist():
    compiled = compiled_kernels()
    for where, names in (("matrix", matrix_kernels()), ("build restatement", set(BUILD_KERNELS)),
                         ("ELSEWHERE", set(ELSEWHERE)), ("UNREACHABLE", set(UNREACHABLE))):
        ghost = sorted(names - compiled)
        assert not ghost, "%s names instantiations the library does not have: %s" % (where, ghost)


def test_every_instantiation_is_named_by_one_row():
    """deleting any row of the matrix then fails test_every_instantiation_has_exactly_one_home"""
    seen = {}
    for row in KM.CASES:
        for k in row.kernels:
            assert k not in seen, "%s is named by two rows: %s and %s" % (k, seen[k], row.kernels)
            seen[k] = row.kernels


def test_the_matrix_table_is_well_formed():
    compiled = compiled_kernels()
    for row in KM.CASES:
        assert row.kernels and all(isinstance(k, str) for k in row.kernels) and row.calls, row
        for c in row.calls:
            assert c.group in KM.GROUPS, c
            assert c.entry in ("batch", "layer", "device", "distance", "brute", "brute_fast", "filtered",
                               "filtered_exact"), c
            assert (c.entry == "layer") == (c.ent > 0), c
            # what a call launches besides its row's kernels exists, and `also` is pinned by some other row
            assert set(c.also) | set(c.may) <= compiled, c
            assert set(c.also) <= matrix_kernels() - set(row.kernels), c
        ids = [KM.call_id(c) for c in row.calls]
        assert len(ids) == len(set(ids)), ("duplicate calls", row.kernels)
