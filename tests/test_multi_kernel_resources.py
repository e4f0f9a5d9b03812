"""The exact-scan kernels (exact_scan.hip) compiled for gfx950 with the Makefile's flags: both instantiations of
hx_distance_kernel -- the distance seam, the MMR selection, the compose and the fusion of multi-vector search are its
four source forms -- run without scratch and without spilled vector registers (no GPU needed: hipcc cross-compiles)."""
import os

import pytest

from tests.kernel_resources import HIPCC, ROOT, resource_usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distance_kernel_has_no_scratch_or_vgpr_spills():
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", "exact_scan.hip")
    assert "fuse_lists<KIND>" in open(src).read(), "the fusion is a source form of hx_distance_kernel"
    kernels, _ = resource_usage("exact_scan.hip")
    seam = {k: v for k, v in kernels.items() if "hx_distance_kernel" in k}
    assert len(seam) == 2 and sum("ILi0E" in k for k in seam) == 1 and sum("ILi1E" in k for k in seam) == 1, sorted(kernels)
    for name, r in seam.items():
        assert "ScratchSize" in r and "VGPRs Spill" in r, (name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r.get("VGPRs", 0) <= 256, (name, r)
