"""Every distance routine against the CPU oracle at the edges of f32's range (tests/numeric_range.py holds the recipes,
the table and the runner): rows and queries scaled so that every squared sum is subnormal (`sub`), has a handful of
bits left and ties everywhere (`under`), or overflows for some rows of a query and not for others (`over`); queries of
signed zeros, subnormal inputs, +-3e38 and a +inf component besides.  Per call: the kernel log names exactly the row's
instantiation(s); ids, distance bits, counts and counters are the oracle's and the status is 0 wherever the oracle
answers; an error status and count 0 exactly where it raises.  tests/test_numeric_range_host.py shows on the CPU that
the recipes do what they claim.  Every test here needs a real MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ground_truth_inputs as G
from tests import kernel_matrix as KM
from tests import numeric_range as NR
from tests.test_ground_truth_inputs import flat_oracle
from tests.test_gpu_ground_truth import flat_product

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kc", [kc for kc in NR.TABLE if kc[1].group == "default"], ids=NR.table_id)
@pytest.mark.parametrize("recipe", NR.RECIPES)
def test_default_routines(recipe, kc):
    NR.run_call(kc[0], kc[1], recipe)


@pytest.mark.parametrize("group", sorted({kc[1].group for kc in NR.TABLE} - {"default"}))
@pytest.mark.parametrize("recipe", NR.RECIPES)
def test_environment_group(recipe, group):
    env = dict(os.environ, **KM.GROUPS[group])
    out = subprocess.run([sys.executable, "-m", "tests.numeric_range", group, recipe], cwd=KM.ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "NUMERIC RANGE OK %s" % group in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])


@pytest.mark.parametrize("recipe", NR.RECIPES)
def test_mfma_scan_hands_the_recipes_to_the_exact_scan(recipe):
    NR.run_brute_fast(recipe)


@pytest.mark.parametrize("log2_scale,fast", [(-50, False), (-48, True), (38, True), (39, False)])
def test_mfma_scan_at_the_edges_of_its_range(log2_scale, fast):
    """integer rows in {0, .., 3} times a power of two: scores exact at any scale that keeps the products normal.  With
    every non-zero |component| at least 2^-48, or at most 3 * 2^38 < 2^40, the screen serves the call; with the largest
    of a row at 3 * 2^-50 or 3 * 2^39 it is the exact scan's.  Either way the answer is the oracle's on every query."""
    X, Q = G.ints(300, 8, 3)
    s = np.float32(2.0 ** log2_scale)
    X, Q = X * s, Q * s
    log = NR.brute_fast_contract(flat_product(X), flat_oracle(X), X, Q, G.K, "ints x 2^%d" % log2_scale, every=True)
    assert log == (NR.FAST_KERNELS if fast else NR.EXACT_KERNELS), log
