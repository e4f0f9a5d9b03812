"""Every walk routine against the CPU oracle on graphs no builder makes (tests/graph_shapes.py holds the recipes, the
table and the runner): ids that all live in the last buckets of the visited table (`collide`), a chain of 1 000 nodes
on two upper layers (`chain`), rows of degree S - 1, S, S + 1 and at the chunk boundaries of the overflow passes on
layer 0 and above (`degrees`), reachable sets of ef - 1, ef, ef + 1 nodes under a tower of sixteen layers (`small`),
and an entry point below the top layer (`misplaced`).  Per call: the kernel log names exactly the row's
instantiation(s); ids, distance bits, counts and counters are the oracle's; `misplaced` is
HNSW_ERR_NODE_NOT_IN_GRAPH for every query.  tests/test_graph_shapes_host.py shows on the CPU that the recipes do what
they claim.  Every test here needs a real MI355X."""
import os
import subprocess
import sys

import pytest

from tests import graph_shapes as GS
from tests import kernel_matrix as KM

pytestmark = pytest.mark.gpu

DEFAULT = [(recipe, kc) for recipe in GS.ALL_RECIPES for kc in GS.TABLE
           if kc[1].group == "default" and recipe in GS.recipes_of(kc[1])]


@pytest.mark.parametrize("recipe,kc", DEFAULT, ids=["%s-%s" % (r, GS.table_id(kc)) for r, kc in DEFAULT])
def test_default_routines(recipe, kc):
    GS.run_call(kc[0], kc[1], recipe)


@pytest.mark.parametrize("group", sorted({kc[1].group for kc in GS.TABLE} - {"default"}))
@pytest.mark.parametrize("recipe", GS.ALL_RECIPES)
def test_environment_group(recipe, group):
    env = dict(os.environ, **KM.GROUPS[group])
    out = subprocess.run([sys.executable, "-m", "tests.graph_shapes", group, recipe], cwd=KM.ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GRAPH SHAPES OK %s" % group in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
