"""The filtered-search kernels (search_filtered.hip) compiled for gfx950: every instantiation runs without scratch
and without spilled vector registers (no GPU needed: hipcc cross-compiles)."""
import os

import pytest

from tests.kernel_resources import HIPCC, resource_usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_filtered_kernels_have_no_scratch_or_spills():
    kernels, _ = resource_usage("search_filtered.hip")
    graph = {k: v for k, v in kernels.items() if "hx_filt_graph_kernel" in k}
    # f32 100d, f32 128d, quant8 100d and the any-dimension forms of both kinds, at one, two and four list registers
    assert len(graph) == 15, sorted(kernels)
    for tag in ("ILi1ELi25ELi100E", "ILi1ELi32ELi128E", "ILi0ELi4ELi100E", "ILi1ELi0ELi0E", "ILi0ELi0ELi0E"):
        assert sum(tag in k for k in graph) == 3, tag
    others = [k for k in kernels if "hx_filt_" in k and k not in graph]
    assert len(others) == 4, sorted(kernels)  # compaction, the scan for both kinds, the merge
    for name, r in kernels.items():
        if "hx_filt_" not in name:
            continue
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy", 0) >= 2, (name, r)
