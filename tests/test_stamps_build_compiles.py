"""The stamps build (make stamps: the in-kernel cycle stamps of stamps.h) still compiles, in both of its flavours, and
keeps its accumulators in registers (no GPU needed: hipcc cross-compiles for gfx950).  Nothing else in the suite
builds it, and every performance change of the lean kernels was steered by it.  A slot that is not a compile-time
constant would move a kernel's accumulator array to scratch: that shows here as ScratchSize != 0.

The commit that gave the slots names had scratch 0 and no spill in every kernel of both files, before and after
(23 kernels in search_lean.hip, 81 in search_kernels.hip), so the same is asserted of every kernel, with no
exception."""
import os

import pytest

from tests.kernel_resources import HIPCC, resource_usage
FLAVOURS = {"stamps": ["-DHX_STAMPS"], "front": ["-DHX_STAMPS", "-DHX_STAMPS_FRONT"]}
# file -> the kernels it must report (a file whose kernels vanished from the remarks would pass the loop below)
KERNELS = {"search_lean": 23, "search_kernels": 81}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_stamps_build_compiles_without_scratch(name, flavour):
    # the Makefile's DEVFLAGS, device side only
    kernels, _ = resource_usage(name + ".hip", ("--cuda-device-only", *FLAVOURS[flavour]), timeout=1800)
    assert len(kernels) == KERNELS[name], sorted(kernels)
    for kname, r in kernels.items():
        assert "ScratchSize" in r and "VGPRs Spill" in r, (kname, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (kname, r)
