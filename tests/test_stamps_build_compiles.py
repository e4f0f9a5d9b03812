"""The stamps build (make stamps: the in-kernel cycle stamps of stamps.h) still compiles, in both of its flavours, and
keeps its accumulators in registers (no GPU needed: hipcc cross-compiles for gfx950).  Nothing else in the suite
builds it, and every performance change of the lean kernels was steered by it.  A slot that is not a compile-time
constant would move a kernel's accumulator array to scratch: that shows here as ScratchSize != 0.

The commit that gave the slots names had scratch 0 and no spill in every kernel of both files, before and after
(23 kernels in search_lean.hip, 81 in search_kernels.hip), so the same is asserted of every kernel, with no
exception."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAVOURS = {"stamps": ["-DHX_STAMPS"], "front": ["-DHX_STAMPS", "-DHX_STAMPS_FRONT"]}
# file -> the kernels it must report (a file whose kernels vanished from the remarks would pass the loop below)
KERNELS = {"search_lean": 23, "search_kernels": 81}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_stamps_build_compiles_without_scratch(tmp_path, name, flavour):
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", name + ".hip")
    # the Makefile's DEVFLAGS, device side only
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
           "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), *FLAVOURS[flavour], "-c", src,
           "-o", str(tmp_path / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(kernels) == KERNELS[name], sorted(kernels)
    for kname, r in kernels.items():
        assert "ScratchSize" in r and "VGPRs Spill" in r, (kname, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (kname, r)
