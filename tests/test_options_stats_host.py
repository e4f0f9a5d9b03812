"""hnsw_set_option and hnsw_get_stat on a fresh empty handle, without a GPU: every name the two tables hold answers,
every other name is refused with its text, and every bounded option is refused just below its bound.  The names are
written out here, not read from the library: a name that leaves a table fails this test."""
import pytest

import hnsw_rs_amd as H
from hnsw_rs_amd import _lib

STATS = [
    "uploads", "point_patches", "patch_fallbacks",
    "build_points", "build_batches", "build_rows_read", "build_adj_rows", "build_adj_ids", "build_records", "build_removals",
    "build_insert_kernel_us", "build_insert_phase_us", "build_connect_us", "build_connect_kernel_us", "build_rows_owned",
    "build_rows_received", "build_exchange_bytes", "build_exchange_us", "build_cpu_path_points", "build_rerun_points",
    "build_kept_last_edges",
    "filtered_queries_graph", "filtered_queries_exact", "filtered_overflow_exact", "label_words_uploaded",
    "filtered_range_calls", "filtered_range_ranges", "filtered_set_range_calls", "filtered_set_range_groups",
    "filtered_one_calls", "filtered_one_batches", "filtered_ranges_calls", "filtered_ranges_groups", "filtered_multi_calls",
    "filtered_multi_masks", "mask_set_words_uploaded", "mask_set_recounts", "mask_set_compactions", "filtered_set_calls",
    "shard_calls", "shard_merges", "grouped_calls", "grouped_launches",
    "deleted", "deleted_mask_words_uploaded", "deleted_queries_graph", "deleted_queries_exact", "deleted_overflow_exact",
    "coalesced_batches", "coalesced_queries", "coalesced_max_batch", "coalesce_ns_window", "coalesce_ns_turn",
    "coalesce_ns_gpu", "coalesce_ns_handout",
]

# name -> (a value inside its bound, [(a value just outside, the refusal)])
OPTIONS = {
    "inline_rows": (-1, []),
    "inline_budget_mb": (65536, []),
    "gpu_build": (0, []),
    "metric_cosine": (0, []),
    "filter_exact_max": (-1, []),
    "filter_exact_grouped": (1, [(-1, "filter_exact_grouped must be 0 or 1"), (2, "filter_exact_grouped must be 0 or 1")]),
    "mask_set_cache_mb": (0, [(-1, "mask_set_cache_mb must not be negative")]),
    "gpu_build_batch_max": (1, [(0, "gpu_build_batch_max must be positive")]),
    "gpu_build_batch_div": (1, [(0, "gpu_build_batch_div must be positive")]),
    "coalesce_us": (-1, []),
    "coalesce_depth": (1, [(0, "coalesce_depth must be positive")]),
    "coalesce_max": (1, [(0, "coalesce_max must be positive")]),
}


def refused(call, text):
    with pytest.raises(H.HnswError) as e:
        call()
    assert e.value.code == _lib.ERR_ARG
    assert _lib.lib().hnsw_last_error() == text.encode(), text


def test_every_statistic_answers_and_no_other_name():
    index = H.HNSW.new(8, 16, 4)
    assert len(set(STATS)) == len(STATS) == 55
    for name in STATS:
        assert index.stat(name) == 0, name
    for name in ("build_", "build_nothing", "", "uploads ", "Uploads", "upload", "points", "build_uploads"):
        refused(lambda: index.stat(name), "unknown statistic %s" % name)


def test_every_option_is_accepted_inside_its_bound_and_refused_below_it():
    index = H.HNSW.new(8, 16, 4)
    for name, (inside, outside) in OPTIONS.items():
        index.set_option(name, inside)
        for value, text in outside:
            refused(lambda: index.set_option(name, value), text)
        index.set_option(name, inside)  # (a refusal leaves the option settable)
    # values above a clamp are stored as the clamp, not refused
    for name in ("mask_set_cache_mb", "gpu_build_batch_max", "gpu_build_batch_div", "coalesce_us", "coalesce_depth", "coalesce_max"):
        index.set_option(name, 1 << 40)
    for name in ("", "inline_rows ", "Inline_rows", "coalesce", "uploads"):
        refused(lambda: index.set_option(name, 1), "unknown option %s" % name)
    clone = index.clone()  # (an empty handle clones, options and all, without a device)
    assert clone.len() == 0
