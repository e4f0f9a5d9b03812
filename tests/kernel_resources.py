"""What the compiler says a kernel file's kernels use: one compile of hnsw_rs_amd/csrc/<source> for gfx950 with the
Makefile's flags and -Rpass-analysis=kernel-resource-usage, the remarks parsed, once per process and set of flags.
Imports nothing of the library: it loads without the built .so."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def resource_usage(source_name, extra_flags=(), timeout=900):
    """({mangled kernel name: {remark: int}}, the compiler's stderr) of hnsw_rs_amd/csrc/<source_name>; extra_flags is a
    tuple of further compiler arguments.  A compile that fails fails the calling test with the tail of stderr."""
    src = os.path.join(ROOT, "hnsw_rs_amd", "csrc", source_name)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
               *extra_flags, "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(tmp, "kernels.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
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
    return kernels, out.stderr
