"""One parity case per reachable search-side kernel instantiation (tests/kernel_matrix.py holds the table): the kernel
launch log must name exactly the row's instantiation(s), and ids, distance bits, counts and counters must equal the
CPU oracle's (filtered rows: tests/filtered_restate.py's).  Every fixture's queries include stored rows, a constant
row, rows plus a large offset and, f32, a row whose distances are all +inf.  Rows of an environment group run in a
child process of their own, one after another.  Every test here needs a real MI355X."""
import os
import subprocess
import sys

import pytest

from tests import kernel_matrix as KM

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [r for r in KM.CASES if any(c.group == "default" for c in r.calls)], ids=KM.case_id)
def test_default_kernels(row):
    KM.run_case(row)


@pytest.mark.parametrize("group", [g for g in KM.GROUPS if g != "default"])
def test_environment_group(group):
    env = dict(os.environ, **KM.GROUPS[group])
    out = subprocess.run([sys.executable, "-m", "tests.kernel_matrix", group], cwd=KM.ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "KERNEL MATRIX OK %s" % group in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
